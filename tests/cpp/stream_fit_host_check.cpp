// stream_fit_host_check.cpp - a plain host program over csrc/mps2qc_resident.h (no HIP): what the host decides before a
// resident streaming fit is launched, printed for tests/test_mps2qc_resident_cpu.py to compare with its own formulas.
//   bitrev n i...            sfd_bitrev(i, n) of every index given
//   bitrev_all n             sfd_bitrev(i, n) for i = 0 .. 2^n - 1
//   opts a b c d             sfd_check_opts of {target_on_device, target_little_endian, check_every, use_graph}: "ok" or "refused <message>"
//   defaults                 sfd_default_opts
//   sizes n G batch          blocks_amp blocks_vec state_count env_partial_count ov_partial_count
//   steps max_iter check     sfd_max_steps_enqueued
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "mps2qc_resident.h"

using namespace mps2qc;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string cmd = argv[1];
  if (cmd == "bitrev" && argc >= 3) {
    const int n = atoi(argv[2]);
    for (int a = 3; a < argc; ++a) printf("%zu\n", sfd_bitrev((size_t)strtoull(argv[a], nullptr, 10), n));
    return 0;
  }
  if (cmd == "bitrev_all" && argc == 3) {
    const int n = atoi(argv[2]);
    for (size_t i = 0; i < ((size_t)1 << n); ++i) printf("%zu\n", sfd_bitrev(i, n));
    return 0;
  }
  if (cmd == "opts" && argc == 6) {
    const mps2qc_resident_opts_t o{atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5])};
    std::string err;
    if (sfd_check_opts(o, err)) printf("ok\n");
    else printf("refused %s\n", err.c_str());
    return 0;
  }
  if (cmd == "defaults") {
    const mps2qc_resident_opts_t o = sfd_default_opts();
    printf("%d %d %d %d\n", o.target_on_device, o.target_little_endian, o.check_every, o.use_graph);
    return 0;
  }
  if (cmd == "sizes" && argc == 5) {
    const int n = atoi(argv[2]), G = atoi(argv[3]), B = atoi(argv[4]);
    printf("%zu %zu %zu %zu %zu\n", sfd_blocks_amp(n), sfd_blocks_vec(n), sfd_state_count(n, B), sfd_env_partial_count(n, G, B),
           sfd_ov_partial_count(n, B));
    return 0;
  }
  if (cmd == "steps" && argc == 4) {
    printf("%lld\n", sfd_max_steps_enqueued(atoi(argv[2]), atoi(argv[3])));
    return 0;
  }
  return 2;
}
