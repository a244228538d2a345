#!/bin/bash
# Full 1-GPU bench line, then a 2-rank gloo rehearsal of the N > 1 path on the
# same GPU (no CPU legs).  usage: tools/bench_check.sh OUT_DIR
set -e
OUT=${1:?usage: tools/bench_check.sh OUT_DIR}
mkdir -p $OUT
timeout -k 10 560 python3 -u bench.py --full > $OUT/n1.log 2>&1
ZKMI_DIST_BACKEND=gloo timeout -k 10 300 python3 -m torch.distributed.run --nnodes=1 --nproc-per-node 2 \
  --master-addr 127.0.0.1 --master-port 29533 bench.py --full --gpus 2 --steps 6 --warmup 2 --no-cpu-baseline --no-zbatch \
  --no-l2 > $OUT/n2_gloo.log 2>&1
