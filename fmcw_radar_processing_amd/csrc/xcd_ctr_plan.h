// Which of the context's two k_rdx counter sets a launch counts in, which one it zeroes for the
// next launch, and which one the launch after it counts in (fmcw_api.cpp process_onepass,
// kernels_xcd.hip launch_xcd).  No HIP types: tests/native/xcd_ctr_plan.cpp checks the rule on the
// host over every sequence of the FMCW_XCD_MEMSET knob.
//
// The rule: a launch counts in set `set`, its block 0 zeroes the other set, and the next launch
// counts in that other set -- with or without the knob.  FMCW_XCD_MEMSET=1 only adds a memset of
// the counting set in front of the launch.  So the knob may change from one launch to the next:
// the set a launch counts in was zeroed by the launch before it (or by the context's first
// allocation), whatever that launch's knob was.
#pragma once

namespace fmcw {

struct XcdCtrPlan {
  int count_set;       // the set (0 / 1) this launch counts in: clean when the launch starts
  int clear_set;       // the set this launch's block 0 zeroes for the next launch, or -1: none
  bool memset_first;   // zero count_set on the stream before the launch
  int next_set;        // the set the next launch counts in
};

inline XcdCtrPlan xcd_ctr_plan(int set, bool memset_knob) {
  return XcdCtrPlan{set, 1 - set, memset_knob, 1 - set};
}

}  // namespace fmcw
