"""The LDS budget of the trace launches (ezrt_amd/csrc/hip/ezrt_lds_budget.h) against recorded values.

tests/golden/lds_budget.npz holds what the three launch configurations computed -- traceq_kernel's, traceq4_kernel's and the count of
records staged that picks the workgroups per CU -- when each spelled the arithmetic out for itself, over a grid: stack rows 1-40,
workgroups per CU 1-8, record sizes 80 and 112 bytes, 0 / 1 / 50 / 10^6 records in the tree, a knob cap of 0 / 64 / 10^6.  Columns:
rows, workgroups wanted, record bytes, records in the tree, cap | workgroups per CU, records staged, LDS bytes of the launch, records
that fit without the caps (-1: not computed for the 80-byte records).  The header needs no HIP include: g++ compiles it into a
stand-alone program here, and every row must match."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <climits>
#include <cstdio>
#include "ezrt_lds_budget.h"
int main() {
  int rows, wgs, rec, n_tree, cap;
  while (scanf("%d %d %d %d %d", &rows, &wgs, &rec, &n_tree, &cap) == 5) {
    const size_t fixed = ((size_t)rows + 1) * 256 * sizeof(int); // stack rows + the lane table, 256 lanes
    const int per_cu = ezi::lds_workgroups(wgs, fixed);
    const int staged = ezi::lds_records(per_cu, fixed, (size_t)rec, n_tree, cap);
    printf("%d %d %zu %d\n", per_cu, staged, fixed + (size_t)staged * (size_t)rec, ezi::lds_records(wgs, fixed, (size_t)rec, INT_MAX, INT_MAX));
  }
}
"""


def test_lds_budget_matches_the_recorded_values(tmp_path):
    rows = np.load(os.path.join(ROOT, "tests", "golden", "lds_budget.npz"))["rows"]
    assert rows.shape == (40 * 8 * 2 * 4 * 3, 9)
    src, exe = tmp_path / "lds_budget.cpp", tmp_path / "lds_budget"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ezrt_amd", "csrc", "hip"),
                    "-o", str(exe), str(src)], check=True)
    text = "".join("%d %d %d %d %d\n" % tuple(r[:5]) for r in rows)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout
    got = np.array([line.split() for line in out.splitlines()], dtype=np.int64)
    assert got.shape == (len(rows), 4)
    uncapped = rows[:, 8] >= 0
    assert uncapped.sum() == len(rows) // 2
    bad = np.flatnonzero((got[:, :3] != rows[:, 5:8]).any(axis=1) | (uncapped & (got[:, 3] != rows[:, 8])))
    assert bad.size == 0, "first mismatch: inputs %s, recorded %s, computed %s" % (rows[bad[0], :5], rows[bad[0], 5:], got[bad[0]])
