/* mps2qc_resident_hip.h - the resident streaming fit of libmps2qc_hip.so; part of the C ABI of mps2qc_hip.h, which
 * includes this file (conventions, error codes and mps2qc_last_error are described there). */
#ifndef MPS2QC_RESIDENT_HIP_H
#define MPS2QC_RESIDENT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The streaming fit with the optimiser on the device too (resident streaming fit): the gates, both moments, the loss
 * history and the termination state of every fit stay in device memory for the whole fit; one step is 2 G + 5 kernel
 * launches and no copy, and the host only replays that sequence and reads the stop flags every check_every steps.  Same
 * arguments up to param_tol, same optimiser and bookkeeping and the same outputs as mps2qc_fit_brickwork_stream (the
 * two agree to rounding, not bit for bit: the update runs in another arithmetic order); loss_history entries at or
 * beyond n_iter are 0; a fit that has stopped is no longer swept, so its final_gates, last_envs and last_overlap are
 * those of its last executed step.
 *   target          host memory, or (target_on_device) device memory of device_id that no other stream is still
 *                   writing; in quimb's order, or (target_little_endian) in the order of libvqe_hip.so - qubit 0 = bit 0,
 *                   e.g. the vector vqe_lanczos_dev leaves - which is bit-reversed on the device while it is copied
 *   steps_enqueued  step sequences put on the stream: a multiple of check_every, at most max_iter rounded up to one
 * VQE_EINVAL (-22), before anything is launched: what mps2qc_fit_brickwork_stream refuses, check_every < 1, a flag
 * outside its listed values, target_on_device = 1 with a pointer that is not device memory of device_id. */
typedef struct { int32_t target_on_device;      /* 0: `target` is host memory; 1: device memory on device_id */
                 int32_t target_little_endian;  /* 0: site 0 = most significant bit (quimb); 1: the engine's order */
                 int32_t check_every;           /* steps between two host reads of the stop flags, >= 1 */
                 int32_t use_graph;             /* -1: as MPS2QC_STREAM_GRAPH says; 0: plain launches; 1: graph */
               } mps2qc_resident_opts_t;
int mps2qc_resident_default_opts(mps2qc_resident_opts_t* o);            /* 0, 0, 8, -1 */
int mps2qc_fit_brickwork_resident(int device_id, int n_qubits, int n_gates, const int32_t* sites,
                                  int batch, const void* target, int target_shared,
                                  const double* init_gates,
                                  double lr, double beta1, double beta2, double eps, int jit_frozen,
                                  int max_iter, double tol, double param_tol,
                                  const mps2qc_resident_opts_t* opts /* NULL: defaults */,
                                  double* opt_gates, double* final_gates, double* loss_history,
                                  double* best_val, int32_t* n_iter,
                                  double* last_envs, double* last_overlap, float* total_ms,
                                  int32_t* steps_enqueued /* or NULL */);

#ifdef __cplusplus
}
#endif
#endif
