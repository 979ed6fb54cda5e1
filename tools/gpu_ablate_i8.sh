#!/bin/bash
# timing-only ablations of k_var_i8: libraries built with -DGPT_ABL_I8=n (make ablate-i8: csrc/build/libgpt_abl_i8_<n>.so, built
# beforehand), selected through GPT_HIP_LIB; outputs of the ablated builds are wrong on purpose (bench sanity check relaxed by
# GPT_BENCH_ABLATE).  Variants: gpt_kvar_i8.h; ABL_I8_SET="0 4 5 7 8" runs a subset (0 is the shipped library).
# usage: tools/gpu_ablate_i8.sh [output directory]
set -u
OUT=${1:-ablate_i8_out}; mkdir -p "$OUT"
B=$PWD/gaussian_process_transportation_amd/csrc/build
for v in ${ABL_I8_SET:-0 1 2 3 4 5 6 7 8}; do
  if [ $v -eq 0 ]; then LIB=$PWD/gaussian_process_transportation_amd/libgpt_hip.so; else LIB=$B/libgpt_abl_i8_$v.so; fi
  [ -f "$LIB" ] || { echo "missing $LIB: run make -C gaussian_process_transportation_amd/csrc ablate-i8 first"; exit 1; }
  GPT_BENCH_ABLATE=1 GPT_HIP_LIB=$LIB timeout -k 10 200 python bench.py --gpus 1 --steps 3 --warmup 2 --cpu-sample 0 > "$OUT/abl$v.log" 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then echo "variant $v ended with $rc: stopping"; exit $rc; fi
  grep '^{' "$OUT/abl$v.log" | python3 -c "import json,sys; d=json.loads(sys.stdin.readline()); print('ABL_I8=$v ms_per_step %.1f var_ms %.1f' % (d['ms_per_step'], d['roofline']['kernel_ms']))"
done
