// stream_noise_grad_check.cpp - the host rules of the streaming form of the noisy gradients (vqe_set_stream_noise_grad,
// DESIGN 4.21) in csrc/noise_grad_host.h without a GPU: the extended verdict and the chunk planner of the (circuit,
// realisation) grid.  tests/test_stream_noise_grad_cpu.py builds it with -fsanitize=address,undefined, runs it as a
// program and compares every printed line with the rules restated there.
//   verdict <n_real> <mode> <pauli> <lds> <stream>   ->  "verdict <v>" (stream < 0: the four-field initialisation)
//   plan <B> <T> <cap>                               ->  "plan <pairs> <resident> <chunks>", then per chunk
//                                                        "chunk <c> <lo> <hi> <b(lo)> <t(lo)> <b(hi-1)> <t(hi-1)>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "noise_grad_host.h"

using namespace vqe;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char op[64];
  long a, b, c, d, e;
  while (fscanf(f, "%63s %ld %ld %ld %ld %ld", op, &a, &b, &c, &d, &e) == 6) {
    if (!strcmp(op, "verdict")) {
      // the aggregate initialisation of the callers that know four fields keeps its meaning
      const NoiseGradState old{(int)a, (int)b, c != 0, d != 0};
      if (old.stream_on) { fclose(f); return 4; }
      const NoiseGradState s = e < 0 ? old : NoiseGradState{(int)a, (int)b, c != 0, d != 0, e != 0};
      printf("verdict %d\n", (int)noise_grad_verdict(s));
    } else if (!strcmp(op, "plan")) {
      const NoiseGradChunks p = noise_grad_chunks((int)a, (int)b, (int64_t)c);
      printf("plan %lld %d %d\n", (long long)p.pairs, p.resident, p.chunks);
      std::vector<int> seen((size_t)p.pairs, 0);
      int64_t next = 0;
      for (int k = 0; k < p.chunks; ++k) {
        int64_t lo, hi;
        noise_grad_chunk_range(p, k, &lo, &hi);
        if (lo != next || hi <= lo || hi - lo > p.resident) { fclose(f); return 5; }      // in order, none empty, none too large
        for (int64_t v = lo; v < hi; ++v) {
          const NoiseGradPair q = noise_grad_pair(v, (int)b);
          if (q.b < 0 || q.b >= a || q.t < 0 || q.t >= b || (int64_t)q.b * b + q.t != v) { fclose(f); return 6; }
          ++seen[(size_t)v];
        }
        const NoiseGradPair first = noise_grad_pair(lo, (int)b), last = noise_grad_pair(hi - 1, (int)b);
        printf("chunk %d %lld %lld %d %d %d %d\n", k, (long long)lo, (long long)hi, first.b, first.t, last.b, last.t);
        next = hi;
      }
      if (next != p.pairs) { fclose(f); return 7; }
      for (int x : seen) if (x != 1) { fclose(f); return 8; }                                // every pair once
      int64_t lo, hi;
      noise_grad_chunk_range(p, p.chunks, &lo, &hi);                                        // past the end: empty
      if (lo != hi) { fclose(f); return 9; }
    } else { fclose(f); return 3; }
  }
  fclose(f);
  puts("ok");
  return 0;
}
