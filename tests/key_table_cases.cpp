// Drives the shared spatial-keying code on the host: the key table's probe loops (csrc/gp_key_table.hpp: key_find / key_claim, the very loops the kernels run -- only
// key_cas differs), the cell rule and the box (csrc/gp_cells.hpp: cell_of, CellBox).  Neither header needs a HIP header.  Built by tests/test_key_table_cpu.py with the
// host compiler and -fsanitize=address,undefined, and run as a plain program: every case prints "ok <name>" or "FAIL <name>: ...", the exit status is the number of
// failures.  With argv[1]: a file of "mask" and then one "key slot" pair per line (tests/golden/key_table_placement.json, flattened by the test) -- the keys are
// claimed one after another with hash_key and must land in the slots the file states.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

static int g_probes = 0;
#define GP_KEY_PROBE() (++g_probes)
#include "gp_cells.hpp"
#include "gp_key_table.hpp"

using gp::kEmptyKey;
typedef unsigned long long u64;

static int g_failed = 0;
#define CHECK(name, cond)                                     \
  do {                                                        \
    if (cond) {                                               \
      printf("ok %s\n", name);                                \
    } else {                                                  \
      printf("FAIL %s: %s (line %d)\n", name, #cond, __LINE__); \
      g_failed++;                                             \
    }                                                         \
  } while (0)

static int find_probes(const std::vector<u64>& t, uint32_t home, u64 key, int* slot) {
  g_probes = 0;
  *slot = gp::key_find(t.data(), (uint32_t)t.size() - 1, home, key);
  return g_probes;
}
static int claim_probes(std::vector<u64>& t, uint32_t home, u64 key, uint32_t* slot, int* claimed) {
  g_probes = 0;
  *claimed = -1;
  *slot = gp::key_claim(t.data(), (uint32_t)t.size() - 1, home, key, claimed);
  return g_probes;
}

static void key_table_cases() {
  int slot, claimed, probes;
  uint32_t s;
  {  // a 1-slot table (mask = 0)
    std::vector<u64> t(1, kEmptyKey);
    CHECK("one slot: find in the empty table", find_probes(t, 0, 7, &slot) == 1 && slot == -1);
    CHECK("one slot: claim", claim_probes(t, 0, 7, &s, &claimed) == 1 && s == 0 && claimed == 1 && t[0] == 7);
    CHECK("one slot: claim the stored key", claim_probes(t, 0, 7, &s, &claimed) == 1 && s == 0 && claimed == 0);
    CHECK("one slot: find the stored key", find_probes(t, 0, 7, &slot) == 1 && slot == 0);
    CHECK("one slot: full, another key is not found", find_probes(t, 0, 8, &slot) == 1 && slot == -1);
    CHECK("one slot: full, another key finds no room", claim_probes(t, 0, 8, &s, &claimed) == 1 && s == 1 && claimed == 0 && t[0] == 7);
  }
  {  // eight slots, every key at home slot 6: the run wraps past the end, 6 7 0 1 2 3 4 5
    std::vector<u64> t(8, kEmptyKey);
    bool placed = true;
    for (u64 k = 0; k < 8; k++) {
      probes = claim_probes(t, 6, 100 + k, &s, &claimed);
      placed = placed && s == ((6 + k) & 7) && claimed == 1 && probes == (int)k + 1;
    }
    CHECK("shared home slot: the keys fill 6 7 0 1 .. 5, one probe more each", placed);
    bool found = true;
    for (u64 k = 0; k < 8; k++) {
      probes = find_probes(t, 6, 100 + k, &slot);
      found = found && slot == (int)((6 + k) & 7) && probes == (int)k + 1;
    }
    CHECK("shared home slot: every key is found across the end", found);
    CHECK("claiming a stored key: the same slot, nothing claimed", claim_probes(t, 6, 103, &s, &claimed) == 4 && s == 1 && claimed == 0);
    // the table is full now and does not hold key 999
    CHECK("full table: claim finds no room after exactly mask + 1 probes", claim_probes(t, 6, 999, &s, &claimed) == 8 && s == 8 && claimed == 0);
    CHECK("full table: find gives -1 after exactly mask + 1 probes", find_probes(t, 6, 999, &slot) == 8 && slot == -1);
    CHECK("full table: the same from another home slot", claim_probes(t, 3, 999, &s, &claimed) == 8 && s == 8 && find_probes(t, 3, 999, &slot) == 8 && slot == -1);
    bool intact = true;
    for (u64 k = 0; k < 8; k++) intact = intact && t[(6 + k) & 7] == 100 + k;
    CHECK("full table: nothing was overwritten", intact);
  }
  {  // a damaged table: the key stored twice -- the first on the probe path counts
    std::vector<u64> t(8, kEmptyKey);
    t[2] = 50, t[3] = 77, t[4] = 51, t[5] = 77;
    CHECK("damaged table: find takes the first copy", find_probes(t, 2, 77, &slot) == 2 && slot == 3);
    CHECK("damaged table: claim takes the first copy", claim_probes(t, 2, 77, &s, &claimed) == 2 && s == 3 && claimed == 0);
    CHECK("damaged table: from a home slot behind the first copy, the second", find_probes(t, 4, 77, &slot) == 2 && slot == 5);
  }
  {  // a free slot ends a find, and is what a claim takes
    std::vector<u64> t(8, kEmptyKey);
    t[1] = 11;
    CHECK("a free slot ends the search", find_probes(t, 1, 12, &slot) == 2 && slot == -1);
    CHECK("a free slot is claimed", claim_probes(t, 1, 12, &s, &claimed) == 2 && s == 2 && claimed == 1 && t[2] == 12);
  }
}

static bool cell_is(double u, bool want_ok, int want) {
  int c[3];
  // the coordinate on each axis in turn, the other two at 0.25 (cell 0); inv = 1 keeps u the product itself
  for (int a = 0; a < 3; a++) {
    const double p[3] = {a == 0 ? u : 0.25, a == 1 ? u : 0.25, a == 2 ? u : 0.25};
    const bool ok = gp::cell_of(p[0], p[1], p[2], 1.0, c[0], c[1], c[2]);
    if (ok != want_ok) return false;
    for (int b = 0; b < 3; b++)
      if (c[b] != (ok && b == a ? want : 0)) return false;
    if (gp::cell_in_range(u) != want_ok) return false;
  }
  return true;
}

static void cell_cases() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double below = std::nextafter(1.0e9, 0.0);
  CHECK("cell_of: u = 1e9 has no cell", cell_is(1.0e9, false, 0));
  CHECK("cell_of: u = -1e9 has no cell", cell_is(-1.0e9, false, 0));
  CHECK("cell_of: nextafter(1e9, 0) has a cell", cell_is(below, true, (int)std::floor(below)) && (int)std::floor(below) == 999999999);
  CHECK("cell_of: -nextafter(1e9, 0) has a cell", cell_is(-below, true, (int)std::floor(-below)) && (int)std::floor(-below) == -1000000000);
  CHECK("cell_of: NaN has no cell", cell_is(nan, false, 0));
  CHECK("cell_of: +inf has no cell", cell_is(inf, false, 0));
  CHECK("cell_of: -inf has no cell", cell_is(-inf, false, 0));
  CHECK("cell_of: -0.0 is in cell 0", cell_is(-0.0, true, (int)std::floor(-0.0)));
  CHECK("cell_of: -1e-300 is in cell -1", cell_is(-1e-300, true, (int)std::floor(-1e-300)) && (int)std::floor(-1e-300) == -1);
  CHECK("cell_of: 0.5 is in cell 0", cell_is(0.5, true, (int)std::floor(0.5)));
  CHECK("cell_of: whole numbers stay", cell_is(-3.0, true, -3) && cell_is(3.0, true, 3));
  int cx, cy, cz;
  // the product decides, not the coordinate: p = 3e8 at inv = 4 is out of range, p = 3.9e9 at inv = 0.25 is in
  CHECK("cell_of: the scaled coordinate decides", !gp::cell_of(3.0e8, 0.0, 0.0, 4.0, cx, cy, cz) && gp::cell_of(3.9e9, -7.5, 2.0, 0.25, cx, cy, cz) &&
                                                    cx == (int)std::floor(3.9e9 * 0.25) && cy == (int)std::floor(-7.5 * 0.25) && cz == 0);
}

static void box_cases() {
  gp::CellBox neutral;
  CHECK("CellBox: the neutral box is empty", neutral.empty());
  int row[6];
  gp::CellBox fold;
  for (int k = 0; k < 5; k++) {
    gp::CellBox().store(row);
    fold.merge(row);
  }
  CHECK("CellBox: folding neutral boxes stays empty", fold.empty());
  const int cells[4][3] = {{5, -2, 9}, {-7, 4, 9}, {0, 0, -11}, {5, 40, 3}};
  gp::CellBox a, b;
  a.add(cells[0]), a.add(cells[1]);
  b.add(cells[2]), b.add(cells[3]);
  CHECK("CellBox: add gives min / max per axis", !a.empty() && a.lo[0] == -7 && a.lo[1] == -2 && a.lo[2] == 9 && a.hi[0] == 5 && a.hi[1] == 4 && a.hi[2] == 9);
  b.store(row);
  a.merge(row);
  neutral.store(row);
  a.merge(row);
  a.store(row);
  CHECK("CellBox: add then fold gives min / max per axis",
        row[0] == -7 && row[1] == -2 && row[2] == -11 && row[3] == 5 && row[4] == 40 && row[5] == 9);
  const int extreme[2][3] = {{-2147483647 - 1, 0, 2147483647}, {2147483647, 0, -2147483647 - 1}};
  gp::CellBox e;
  e.add(extreme[0]), e.add(extreme[1]);
  CHECK("CellBox: the int range's ends", !e.empty() && e.lo[0] == -2147483647 - 1 && e.hi[0] == 2147483647 && e.lo[2] == -2147483647 - 1 && e.hi[2] == 2147483647);
}

static int placement_case(const char* path) {
  FILE* in = fopen(path, "r");
  if (!in) return 2;
  unsigned mask = 0;
  if (fscanf(in, "%u", &mask) != 1 || (mask & (mask + 1)) != 0) return 2;
  std::vector<u64> table((size_t)mask + 1, kEmptyKey);
  u64 key;
  unsigned want;
  int n = 0;
  bool same = true;
  while (fscanf(in, "%llu %u", &key, &want) == 2) {
    int claimed;
    const uint32_t s = gp::key_claim(table.data(), mask, gp::hash_key(key) & mask, key, &claimed);
    same = same && s == want && claimed == 1;
    printf("placed %llu %u\n", key, s);
    n++;
  }
  fclose(in);
  CHECK("placement: the keys land where the restatement puts them", same && n > 0);
  return 0;
}

int main(int argc, char** argv) {
  key_table_cases();
  cell_cases();
  box_cases();
  if (argc > 1 && placement_case(argv[1]) != 0) return 100;
  return g_failed;
}
