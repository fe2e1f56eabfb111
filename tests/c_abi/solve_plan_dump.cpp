// Executes the K1 solve launcher's decision (csrc/msnap_solve_plan.h: plan_solve, solve_plan_name) on the host and
// prints it, for tests/test_solve_exact_cpu.py.  Plain C++17: no GPU, no HIP.
//     solve_plan_dump <n_cu>
// First line: "consts" and the constants the checks need.  Then one tab-separated line per (order, drones, segments,
// option set): order n m opts n_cu family name instance waves tiles grid block lds slab -- `name` is the
// msnap_last_kernel string, `instance` the kernel template instance (the twist family's carries its wave count).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msnap_solve_plan.h"

using namespace msnap;

struct OptionSet {
  const char *label;
  SolveKnobs k;   // n_cu is filled in per run
};

int main(int argc, char **argv) {
  if (argc != 2 || atoi(argv[1]) < 1) {
    fprintf(stderr, "usage: solve_plan_dump <n_cu>\n");
    return 2;
  }
  const int n_cu = atoi(argv[1]);
  auto knobs = [](int no_twist, int no_twin, int twist_max, int twin_max, int waves, int grid_waves) {
    return SolveKnobs{0, no_twist, no_twin, twist_max, twin_max, waves, grid_waves};
  };
  const OptionSet sets[] = {
      {"", knobs(0, 0, 0, 0, 0, 0)},
      {"no_twist", knobs(1, 0, 0, 0, 0, 0)},
      {"no_twist,no_twin", knobs(1, 1, 0, 0, 0, 0)},
      {"twist_waves=1", knobs(0, 0, 0, 0, 1, 0)},
      {"twist_waves=2", knobs(0, 0, 0, 0, 2, 0)},
      {"twist_waves=4", knobs(0, 0, 0, 0, 4, 0)},
      {"twist_max_drones=1", knobs(0, 0, 1, 0, 0, 0)},
      {"twist_max_drones=4096", knobs(0, 0, 4096, 0, 0, 0)},
      {"twin_max_drones=1", knobs(0, 0, 0, 1, 0, 0)},
      {"twin_max_drones=1048576", knobs(0, 0, 0, 1048576, 0, 0)},
      {"solve_grid_waves=1", knobs(0, 0, 0, 0, 0, 1)},
      {"solve_grid_waves=3", knobs(0, 0, 0, 0, 0, 3)},
      {"no_twist,solve_grid_waves=3", knobs(1, 0, 0, 0, 0, 3)},
      {"no_twist,no_twin,solve_grid_waves=3", knobs(1, 1, 0, 0, 0, 3)},
  };
  const int drones[] = {1, 3, 7, 8, 9, 16, 17, 255, 256, 257, 2048, 2049, 8192, 8193, 65536, 65537, 1048576};
  static const char *const family[] = {"twist", "twin", "reg", "rolled"};
  printf("consts\tkMaxLdsBytes=%zu\tkWave=%d\tkRegMaxSeg=%d\n", kMaxLdsBytes, kWave, kRegMaxSeg);
  const int orders[] = {7, 9};
  for (int order : orders)
    for (const OptionSet &s : sets)
      for (int n : drones)
        for (int m = 1; m <= 200; ++m) {
          if (m > 64 && s.label[0]) continue;   // the long paths: default options only
          SolveKnobs k = s.k;
          k.n_cu = n_cu;
          const SolvePlan p = plan_solve(k, (order + 1) / 2, n, m);
          char name[96], instance[112];
          solve_plan_name(p, name, sizeof(name));
          // the last-kernel string names the instance but for the twist family's wave count
          const char *at = strstr(name, "::");
          snprintf(instance, sizeof(instance), "%s", at ? at + 2 : name);
          if (p.family == SolveFamily::twist) {
            const size_t len = strlen(instance);
            snprintf(instance + len - 1, sizeof(instance) - len + 1, ", %d>", p.waves);
          }
          printf("%d\t%d\t%d\t%s\t%d\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%zu\t%zu\n", order, n, m, s.label, n_cu,
                 family[(int)p.family], name, instance, p.waves, p.tiles, p.grid, p.block, p.lds_bytes, p.slab_bytes);
        }
  return 0;
}
