// Drives gp::shard_layout, gp::gather_send_offset and gp::balanced_boundaries (csrc/gp_shard_layout.hpp, which includes no HIP header) -- the one description of
// which factors a shard of the multi-GPU batch holds, and the balanced contiguous plan -- through scripted cases and prints what they decide.  Built by
// tests/test_shard_layout_cpu.py with the host compiler and -fsanitize=address,undefined, and run as a plain program.  Every input array is sized exactly, so that a
// read past the assignment or the weights is a sanitizer report.
//
// Input (argv[1]), one case per line:
//   L  F  N  width  shard_of[F]     ->  "refused: <reason>" or "rows=<gather rows> | first=<row> contiguous=<0/1> offset=<send offset> index=<ints> | ..." (one group per shard)
//   B  n  k  w[n]                   ->  "begin=<k + 1 ints>"
#include <cstdint>
#include <cstdio>
#include <memory>

#include "gp_shard_layout.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 2;
  char kind = 0;
  while (fscanf(in, " %c", &kind) == 1) {
    if (kind == 'L') {
      int F = 0, N = 0, width = 0;
      if (fscanf(in, "%d %d %d", &F, &N, &width) != 3 || F < 0 || N <= 0 || width <= 0) return 3;
      std::unique_ptr<int[]> shard_of(new int[(size_t)F]);  // exact size (a vector's capacity may hide an overrun)
      for (int i = 0; i < F; i++)
        if (fscanf(in, "%d", &shard_of[(size_t)i]) != 1) return 3;
      gp::ShardLayout L;
      const char* reason = nullptr;
      if (gp::shard_layout(F ? shard_of.get() : nullptr, F, N, &L, &reason) != GP_OK) {
        printf("refused: %s\n", reason);
        continue;
      }
      if ((int)L.shards.size() != N) return 4;
      printf("rows=%zu", L.gather_rows);
      for (const gp::ShardRows& s : L.shards) {
        printf(" | first=%d contiguous=%d offset=%zu index=", s.first_row, s.contiguous ? 1 : 0, gp::gather_send_offset(s, width));
        for (int v : s.index) printf("%d ", v);
      }
      printf("\n");
    } else if (kind == 'B') {
      int n = 0, k = 0;
      if (fscanf(in, "%d %d", &n, &k) != 2 || n < 0 || k <= 0) return 3;
      std::unique_ptr<int64_t[]> w(new int64_t[(size_t)n]);
      for (int i = 0; i < n; i++) {
        long long v = 0;
        if (fscanf(in, "%lld", &v) != 1) return 3;
        w[(size_t)i] = v;
      }
      printf("begin=");
      for (int b : gp::balanced_boundaries(n ? w.get() : nullptr, n, k)) printf("%d ", b);
      printf("\n");
    } else {
      return 3;
    }
  }
  fclose(in);
  return 0;
}
