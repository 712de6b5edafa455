// Drives gp_corr_update (csrc/gp_corr_update.hpp, which includes no HIP header) through scripted cases the way the single factors' linearise and error
// evaluation do (gp_corr_tile.hpp: corr_factor_linearize / corr_factor_compute_error), and prints every decision.  Built by tests/test_corr_update_cpu.py with
// the host compiler and -fsanitize=address,undefined, and run as a plain program.
//
// Input (argv[1]), one command per line, numbers as C99 hexadecimal floats:
//   N <name>            a fresh factor
//   T <rot> <trans>     set_correspondence_update_tolerance
//   L <16 doubles>      a linearise at the column-major pose        -> "L keep=<0|1>"
//   E <16 doubles>      an error evaluation with this pose_lin      -> "E stored=<0|1> lin_valid=<0|1>"  (lin_valid: after the call)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gp_corr_update.hpp"

static bool read_doubles(char* s, int count, double* out) {
  for (int i = 0; i < count; i++) {
    char* end = nullptr;
    out[i] = strtod(s, &end);
    if (end == s) return false;
    s = end;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 2;
  gp_corr_update u;
  char line[1024];
  double v[16];
  int rc = 0;
  while (rc == 0 && fgets(line, sizeof(line), in)) {
    switch (line[0]) {
      case 'N':
        u = gp_corr_update{};
        printf("%s", line);
        break;
      case 'T':
        if (!read_doubles(line + 1, 2, v)) rc = 3;
        u.tol_rot = v[0], u.tol_trans = v[1];
        break;
      case 'L': {
        if (!read_doubles(line + 1, 16, v)) rc = 3;
        const bool keep = u.keep(v);
        if (!keep) u.note_search(v);
        u.note_linearize(v);
        printf("L keep=%d\n", (int)keep);
        break;
      }
      case 'E': {
        if (!read_doubles(line + 1, 16, v)) rc = 3;
        const bool stored = u.stored(v);
        if (!stored) u.note_search(v);
        printf("E stored=%d lin_valid=%d\n", (int)stored, (int)u.lin_valid);
        break;
      }
      default:
        rc = 3;
    }
  }
  fclose(in);
  return rc;
}
