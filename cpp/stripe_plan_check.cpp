/* stripe_plan_check — CPU-runnable check of the striped gather's pure host
 * functions (plan_stripe and the task decode the kernel runs), meant to be
 * built together with csrc/nts_hip.hip under host sanitizers:
 *
 *   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
 *     -Xarch_host -fsanitize=address,undefined \
 *     neutronstarlite_amd/csrc/nts_hip.hip cpp/stripe_plan_check.cpp \
 *     -o stripe_plan_check && ./stripe_plan_check
 *
 * It makes no HIP call, so it needs no device.  For every shape it plans a
 * forced striped launch, decodes every wave slot and requires that each live
 * (work item, first column) comes out exactly once with the right column
 * bound, and nothing else.  Exit 0 on success.
 */
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "../include/nts_hip.h"

static int fail(const char *what, unsigned n, unsigned f, unsigned sf) {
  fprintf(stderr, "stripe_plan_check FAIL: %s (n_items %u f %u stripe %u)\n",
          what, n, f, sf);
  return 1;
}

int main() {
  const unsigned items[] = {1, 7, 8, 9, 1000, 1001};
  const unsigned widths[] = {32, 130, 602, 608};
  const unsigned stripes[] = {16, 32, 64, 128};
  const int runs[] = {0, 3, 17};
  const unsigned window = 128;
  long checked = 0;
  for (unsigned n : items)
    for (unsigned f : widths)
      for (unsigned sf : stripes)
        for (int run : runs) {
          int grid = 0, stripe = 0, per_wave = 0, staged = 0;
          nts_gather_stripe_plan(f, 4, 16, 16, n, n, n, NTS_SCHED_PHASE,
                                 (int)window, 1, (int)sf, run, &staged,
                                 nullptr, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, &grid, nullptr, &stripe, nullptr,
                                 nullptr, nullptr, &per_wave);
          if (!staged || stripe != (int)sf || grid < 8 || grid % 8 ||
              per_wave < (run ? run : 1))
            return fail("plan", n, f, sf);
          const unsigned long long slots =
              (unsigned long long)grid * 4 * per_wave;
          std::vector<nts_vid> it(slots + 16), c0(slots + 16), c1(slots + 16);
          const long long live = nts_gather_stripe_task(
              f, 4, 16, 16, n, n, n, NTS_SCHED_PHASE, (int)window, 1, (int)sf,
              run, n, 0, slots + 16, it.data(), c0.data(), c1.data());
          std::set<std::pair<nts_vid, nts_vid>> seen;
          for (unsigned long long k = 0; k < slots + 16; ++k) {
            if (c0[k] >= c1[k]) continue;
            if (k >= slots) return fail("task past the grid", n, f, sf);
            const nts_vid bound = c0[k] + sf < f ? c0[k] + sf : f;
            if (it[k] >= n || c0[k] >= f || c0[k] % sf || c1[k] != bound)
              return fail("task outside the rows", n, f, sf);
            if (!seen.insert({it[k], c0[k]}).second)
              return fail("task twice", n, f, sf);
          }
          const unsigned long long want =
              (unsigned long long)n * ((f + sf - 1) / sf);
          if ((unsigned long long)live != want || seen.size() != want)
            return fail("tasks missing", n, f, sf);
          ++checked;
        }
  printf("stripe_plan_check ok (%ld launches)\n", checked);
  return 0;
}
