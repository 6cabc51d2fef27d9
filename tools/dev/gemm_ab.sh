#!/bin/bash
# A/B of the blocked-GEMM convolution kernel (YS_NO_GEMM=1 = previous kernels) on the wide-layer configurations + the headline one
O=${TRIAGE_OUT:-triage_out}/gemm; mkdir -p $O
run() { # name, env, args
  env $2 python bench.py --full --steps 6 --warmup 3 --no-cpu-baseline --no-nms --no-infer $3 --dump-launches $O/l_$1.csv 2>$O/$1.err | tail -1 > $O/$1.json
  python -c "import sys,json; d=json.loads(open('$O/$1.json').read()); print('$1', d['value'], d['ms_per_step'], d['roofline']['class_ms_per_step'], d['loss_items'])"
}
run c5_gemm "A=1" "--size x --imgsz 1280 --batch 16"
run c5_old "YS_NO_GEMM=1" "--size x --imgsz 1280 --batch 16"
run c4_gemm "A=1" "--family 11 --size m --task segment --batch 32"
run c4_old "YS_NO_GEMM=1" "--family 11 --size m --task segment --batch 32"
run c2_gemm "A=1" ""
run c2_old "YS_NO_GEMM=1" ""
run c3_gemm "A=1" "--size s --batch 32"
run c3_old "YS_NO_GEMM=1" "--size s --batch 32"
