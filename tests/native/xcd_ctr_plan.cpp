// Host check of the k_rdx counter-set rule (fmcw_radar_processing_amd/csrc/xcd_ctr_plan.h).
//
// A context holds two counter sets.  Each is modelled as clean (all zero) or dirty.  A launch
//   1. zeroes its counting set first when the plan says memset_first,
//   2. must then find its counting set clean (ready counters, member tickets and the abort word all
//      start at zero: a dirty set means consumers that do not wait, or "more than 32 workgroups"),
//   3. leaves its counting set dirty,
//   4. zeroes clear_set (its block 0; never the set it counts in),
// and the next launch counts in next_set.  Every sequence of the FMCW_XCD_MEMSET knob (0 / 1 per
// launch) up to length 10 is run from every start state a context can be in: the next set 0 or 1
// (clean), the other set clean (a new context) or dirty (after any launch).
//
//   xcd_ctr_plan            checks fmcw::xcd_ctr_plan, exit 0 and "ok" when every sequence holds
//   xcd_ctr_plan --parent   checks the rule this one replaced (memset launches always in set 0, no
//                           zeroing of the other set, no toggle): it must be reported as broken,
//                           which shows that the check can fail
#include <cstdio>
#include <cstring>

#include "../../fmcw_radar_processing_amd/csrc/xcd_ctr_plan.h"

namespace {

fmcw::XcdCtrPlan parent_plan(int set, bool memset_knob) {
  if (memset_knob) return fmcw::XcdCtrPlan{0, -1, true, set};
  return fmcw::XcdCtrPlan{set, 1 - set, false, 1 - set};
}

constexpr int MAXLEN = 10;

// 0 when the sequence holds, else the 1-based launch that broke it (what: why)
int run(bool parent, int set, bool other_clean, unsigned knobs, int len, const char** what) {
  bool clean[2];
  clean[set] = true;
  clean[1 - set] = other_clean;
  for (int i = 0; i < len; ++i) {
    const bool knob = (knobs >> i) & 1u;
    const fmcw::XcdCtrPlan p = parent ? parent_plan(set, knob) : fmcw::xcd_ctr_plan(set, knob);
    if (p.count_set < 0 || p.count_set > 1 || p.clear_set < -1 || p.clear_set > 1 || p.next_set < 0 || p.next_set > 1) {
      *what = "a set index out of range";
      return i + 1;
    }
    if (p.memset_first) clean[p.count_set] = true;
    if (!clean[p.count_set]) {
      *what = "counts in a dirty set";
      return i + 1;
    }
    clean[p.count_set] = false;
    if (p.clear_set >= 0) clean[p.clear_set] = true;
    if (clean[p.count_set]) {             // it zeroed the set it counts in, under its own members
      *what = "leaves its counting set clean";
      return i + 1;
    }
    set = p.next_set;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const bool parent = argc > 1 && std::strcmp(argv[1], "--parent") == 0;
  long n = 0;
  for (int len = 1; len <= MAXLEN; ++len)
    for (unsigned knobs = 0; knobs < (1u << len); ++knobs)
      for (int set = 0; set < 2; ++set)
        for (int oc = 0; oc < 2; ++oc) {
          const char* what = "";
          const int bad = run(parent, set, oc != 0, knobs, len, &what);
          ++n;
          if (!bad) continue;
          std::printf("FAIL (%s rule): start set %d, other set %s, knob sequence", parent ? "parent" : "current", set,
                      oc ? "clean" : "dirty");
          for (int i = 0; i < len; ++i) std::printf(" %u", (knobs >> i) & 1u);
          std::printf(": launch %d %s\n", bad, what);
          return 1;
        }
  std::printf("ok (%s rule): %ld knob sequences up to length %d, every launch counted in a clean set\n",
              parent ? "parent" : "current", n, MAXLEN);
  return 0;
}
