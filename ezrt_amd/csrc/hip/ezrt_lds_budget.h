// ezrt_lds_budget.h -- how much of a trace launch's LDS goes to top-of-tree records.  Pure functions of integers with no HIP
// include, so that a host compiler alone can check them (tests/test_lds_budget.py pins them to recorded values).
// A workgroup's LDS is a fixed part (traversal stack + lane table) and as many records as fit beside it when `wgs_per_cu`
// workgroups share the CU's LDS.
#pragma once
#include <cstddef>

namespace ezi {
constexpr size_t LDS_PER_CU = 158 * 1024;    // what the workgroups resident on a CU share
constexpr size_t LDS_PER_LAUNCH = 64 * 1024; // static cap of a dynamic-LDS launch without opt-in

// the workgroups per CU a launch can ask for: as many as wanted, unless their fixed parts alone would not fit
inline int lds_workgroups(int wgs_per_cu, size_t fixed_bytes) {
  if ((size_t)wgs_per_cu * fixed_bytes > LDS_PER_CU) wgs_per_cu = (int)(LDS_PER_CU / fixed_bytes);
  return wgs_per_cu < 1 ? 1 : wgs_per_cu;
}
// the records of `rec_bytes` a workgroup stages beside its fixed part at `wgs_per_cu` workgroups per CU, at most cap_a and cap_b
// (the tree's records, the knob lds_nodes)
inline int lds_records(int wgs_per_cu, size_t fixed_bytes, size_t rec_bytes, int cap_a, int cap_b) {
  size_t budget = LDS_PER_CU / (size_t)(wgs_per_cu > 0 ? wgs_per_cu : 1);
  if (budget > LDS_PER_LAUNCH) budget = LDS_PER_LAUNCH;
  budget -= budget / 16; // allocation-granule slack: a workgroup must not lose its CU slot to rounding
  int n = budget > fixed_bytes ? (int)((budget - fixed_bytes) / rec_bytes) : 0;
  if (n > cap_a) n = cap_a;
  if (n > cap_b) n = cap_b;
  return n < 0 ? 0 : n;
}
} // namespace ezi
