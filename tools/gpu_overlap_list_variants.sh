#!/bin/bash
# tools/gpu_overlap_list_variants.sh [OUT]: the overlap lists (include/ezrt_overlap_list.h) under other compiled limits, on the GPU.
# Build first: `make hip olvariants` (build_ab/libezrt_hip_{i16_t4096,i64_t4096,i0_t2048,i0_t8192,nosort}.so).
#  1. tests/test_gpu_overlap_list.py against the insert_max = 16 library: the seam tests place rows around the limits the loaded
#     library reports, so this is what runs fill_rows' insertion path, which the compiled insert_max = 0 never takes.
#  2. tools/overlap_list_rates.py on the product library (first and last), on the library without the sort launch and on the four
#     variants, each in a process of its own, one JSON line each into OUT/rates.txt (profiles/r25/overlap_list_rates.txt).
# Every step has a time limit of its own, and the script ends at the first step that fails.
R=$(cd "$(dirname "$0")/.." && pwd); O=${1:-$R/build_ab/overlap_list}; mkdir -p "$O"; cd "$R" || exit 1
EZRT_HIP_LIB=$R/build_ab/libezrt_hip_i16_t4096.so timeout -k 10 420 python3 -m pytest -q -m gpu tests/test_gpu_overlap_list.py > "$O/tests_i16.log" 2>&1
rc=$?; tail -3 "$O/tests_i16.log"; [ $rc -eq 0 ] || exit $rc
: > "$O/rates.txt"
for v in product nosort i16_t4096 i64_t4096 i0_t2048 i0_t8192 product_again; do
  lib=$R/build_ab/libezrt_hip_$v.so
  case $v in product*) lib=$R/ezrt_amd/lib/libezrt_hip.so;; esac
  EZRT_HIP_LIB=$lib timeout -k 10 240 python3 tools/overlap_list_rates.py --label $v >> "$O/rates.txt" 2> "$O/rates_$v.err"
  rc=$?; echo "rates $v rc=$rc"
  if [ $rc -ne 0 ]; then tail -5 "$O/rates_$v.err"; exit $rc; fi
done
