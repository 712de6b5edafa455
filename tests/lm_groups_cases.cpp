// Drives gp::lm_layout (csrc/gp_lm_groups.hpp, which includes no HIP header) -- the pair validation, the slot assignment and the record offsets of the
// device-resident LM graph's one create path -- through scripted cases and prints what it decides.  Built by tests/test_lm_groups_cpu.py with the host compiler
// and -fsanitize=address,undefined, and run as a plain program.  Every array is sized exactly, so that a read past a group's pairs or a write past the slot table is
// a sanitizer report.
//
// Input (argv[1]), one case per line of integers:
//   N  held[N]  F  pairs[2F]  G  pairs[2G]  P  (kind a b)[P]
// Output per case: "refused: <message>" or "slots=<n> offsets=<o0> <o1> <o2> records=<R> slot=<N ints> factor_slots=<2R ints>"
#include <cstdio>
#include <memory>
#include <vector>

#include "gp_lm_groups.hpp"

static bool read_ints(FILE* in, size_t count, std::vector<int>* out) {
  out->resize(count);
  for (size_t i = 0; i < count; i++)
    if (fscanf(in, "%d", &(*out)[i]) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 2;
  int N = 0, rc = 0;
  while (rc == 0 && fscanf(in, "%d", &N) == 1) {
    std::vector<int> held, pairs[gp::kLmGroups], pf;
    int count[gp::kLmGroups] = {0, 0}, P = 0;
    if (N < 0 || !read_ints(in, (size_t)N, &held)) rc = 3;
    for (int k = 0; k < gp::kLmGroups && rc == 0; k++)
      if (fscanf(in, "%d", &count[k]) != 1 || count[k] < 0 || !read_ints(in, 2 * (size_t)count[k], &pairs[k])) rc = 3;
    if (rc == 0 && (fscanf(in, "%d", &P) != 1 || P < 0 || !read_ints(in, 3 * (size_t)P, &pf))) rc = 3;
    if (rc != 0) break;
    // exact-size heap copies (a vector's capacity may hide an overrun)
    std::unique_ptr<unsigned char[]> fixed(new unsigned char[(size_t)N]);
    for (int i = 0; i < N; i++) fixed[(size_t)i] = (unsigned char)held[(size_t)i];
    std::unique_ptr<int[]> exact[gp::kLmGroups];
    const int* ptrs[gp::kLmGroups];
    for (int k = 0; k < gp::kLmGroups; k++) {
      exact[k].reset(new int[2 * (size_t)count[k]]);
      for (size_t i = 0; i < 2 * (size_t)count[k]; i++) exact[k][i] = pairs[k][i];
      ptrs[k] = count[k] ? exact[k].get() : nullptr;
    }
    std::unique_ptr<gp_pose_factor[]> factors(new gp_pose_factor[(size_t)P]());
    for (int p = 0; p < P; p++) factors[(size_t)p].kind = pf[3 * (size_t)p], factors[(size_t)p].pose_a = pf[3 * (size_t)p + 1], factors[(size_t)p].pose_b = pf[3 * (size_t)p + 2];
    gp::LmLayout L;
    const std::string refusal = gp::lm_layout(ptrs, count, P ? factors.get() : nullptr, P, N, N ? fixed.get() : nullptr, &L);
    if (!refusal.empty()) {
      printf("refused: %s\n", refusal.c_str());
      continue;
    }
    printf("slots=%d offsets=%d %d %d records=%d slot=", L.slots, L.record_offset[0], L.record_offset[1], L.record_offset[2], L.num_records);
    for (int v : L.slot) printf("%d ", v);
    printf("factor_slots=");
    for (int v : L.factor_slots) printf("%d ", v);
    printf("\n");
  }
  fclose(in);
  return rc;
}
