// vqe_qjump.hip - the kernels of vqe_qjump.h and their launcher, in a translation unit of their own (see qj_launch).
#define VQE_QJUMP_KERNELS
#include "vqe_qjump.h"
#include "vqe_stream_qjump.h"      // the streaming path's trajectory kernels share the helpers above

#include <algorithm>
#include <utility>

namespace vqe {
namespace {

template <int N>
int launch_traj(const BatchArgs& A, const GradHam& GH, const QjDev& Q, int lds_per_cu, int cu_count, hipStream_t stream,
                int* grid_out, int* wg_per_cu_out, hipError_t* err) {
  const size_t lds = qj_lds_bytes(N, A.max_ops, A.max_params);
  if (lds > (size_t)lds_per_cu) return QJ_ETOOLARGE;
  if ((*err = hipFuncSetAttribute((const void*)k_qj_traj<N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess)
    return QJ_EHIP;
  // a persistent grid when B * T exceeds what the device holds
  const int wg_per_cu = std::max(1, std::min(Geo<N>::NT == 64 ? 16 : 8, (int)((size_t)lds_per_cu / lds)));
  const long long total = (long long)A.batch * Q.T;
  const int grid = (int)std::min<long long>(total, (long long)cu_count * wg_per_cu);
  *grid_out = grid;
  *wg_per_cu_out = wg_per_cu;
  hipLaunchKernelGGL(k_qj_traj<N>, dim3((unsigned)grid), dim3(Geo<N>::NT), lds, stream, A, GH, Q);
  return (*err = hipGetLastError()) == hipSuccess ? QJ_OK : QJ_EHIP;
}

template <int... Ns>
int dispatch(std::integer_sequence<int, Ns...>, int n, const BatchArgs& A, const GradHam& GH, const QjDev& Q, int lds_per_cu,
             int cu_count, hipStream_t stream, int* grid, int* wg_per_cu, hipError_t* err) {
  int rc = QJ_ESIZE;
  (void)(... || (n == Ns && ((rc = launch_traj<Ns>(A, GH, Q, lds_per_cu, cu_count, stream, grid, wg_per_cu, err)), true)));
  return rc;
}

}  // namespace

int qj_launch(const BatchArgs& A, const GradHam& GH, const QjDev& Q, int32_t* nfev, long long* jsum, int lds_per_cu,
              int cu_count, hipStream_t stream, int* grid, int* wg_per_cu, hipError_t* err) {
  *err = hipSuccess;
  const int rc = dispatch(std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13>{}, A.n, A, GH, Q, lds_per_cu, cu_count,
                          stream, grid, wg_per_cu, err);
  if (rc != QJ_OK) return rc;
  hipLaunchKernelGGL(k_qj_mean, dim3((unsigned)((A.batch + 63) / 64)), dim3(64), 0, stream, A.batch, Q.T, (const double*)Q.etraj,
                     (const int32_t*)Q.jumps, Q.active, A.noise, Q.eval_id, A.fout, nfev, jsum);
  return (*err = hipGetLastError()) == hipSuccess ? QJ_OK : QJ_EHIP;
}

}  // namespace vqe
