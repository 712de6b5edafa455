#!/bin/bash
# functional rehearsal of the multi-rank bench path on a 1-GPU box: N ranks share the GPU, gloo instead of RCCL
set -u
export TMPDIR=/tmp HSA_ENABLE_IPC_MODE_LEGACY=0 GP_BENCH_BACKEND=gloo
O=${1:-rehearsal_out}
mkdir -p $O
for n in 2 4; do
  timeout 900 python -m torch.distributed.run --nnodes=1 --nproc-per-node $n --master-addr 127.0.0.1 --master-port $((29500 + n)) bench.py --full --gpus $n --steps 50 --warmup 5 --no-cpu-baseline --c4-steps 5 > $O/r02_rehearsal_n$n.log 2>&1
  echo "rehearsal $n exit $?" >> $O/r02_rehearsal_n$n.log
  grep "^{" $O/r02_rehearsal_n$n.log | cut -c1-200; tail -1 $O/r02_rehearsal_n$n.log
done
