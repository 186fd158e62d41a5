#!/bin/bash
# round 6, final kernels: every profile set of the round in one GPU session (run through gpurun)
R=$GRAFT_REPO_ROOT
cd $R
export PROFILE_OUT=${PROFILE_OUT:-$R/profile_out}; mkdir -p $PROFILE_OUT   # where every file of the session lands (git ignores the default)
(timeout 1500 python -m pytest tests -m gpu -q 2>&1 | tail -3) > $PROFILE_OUT/r06_gputest_tail.txt
bash $R/profiles/collect_profiles.sh r06 c2 c3 c4 c5 c6 k6 c7 c8 c9
cd $R
timeout 600 python scripts/decompose_step.py --out $PROFILE_OUT/r06_step_decomposition.json > $PROFILE_OUT/r06_decomp.log 2>&1 < /dev/null
rm -f $PROFILE_OUT/r06_sweep.jsonl
for c in c2 c3; do timeout 600 python bench.py --config $c --steps 50 --warmup 5 --repeats 1 --configs none --no-cpu-baseline --no-variants --full --no-verify --sweep --sweep-out $PROFILE_OUT/r06_sweep.jsonl > /dev/null 2> $PROFILE_OUT/r06_sweep_$c.err < /dev/null; done
bash profiles/collect_sq.sh r06 c2 inst SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVES
bash profiles/collect_sq.sh r06 c5 inst SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVES
rm -f $PROFILE_OUT/r06_inplace.jsonl
timeout 600 python scripts/time_inplace.py --out $PROFILE_OUT/r06_inplace.jsonl > /dev/null 2> $PROFILE_OUT/r06_inplace.err < /dev/null
timeout 900 python scripts/time_shapes.py --out $PROFILE_OUT/r06_shapes.jsonl > /dev/null 2> $PROFILE_OUT/r06_shapes.err < /dev/null
timeout 900 python scripts/stress_rolling.py 200 $PROFILE_OUT/r06_stress_rolling.json > $PROFILE_OUT/r06_stress_rolling.log 2>&1 < /dev/null
timeout 1200 python scripts/stress_parity.py 1500 $PROFILE_OUT/r06_stress_parity.json > $PROFILE_OUT/r06_stress_parity.log 2>&1 < /dev/null
timeout 1200 python scripts/stress_masks.py 400 $PROFILE_OUT/r06_stress_masks.json > $PROFILE_OUT/r06_stress_masks.log 2>&1 < /dev/null
SECONDS=0
python bench.py --gpus 1 --steps 20 --warmup 5 --full > $PROFILE_OUT/r06_default_bench.json 2> $PROFILE_OUT/r06_default_bench.err < /dev/null
echo "default bench: $SECONDS s" >> $PROFILE_OUT/r06_gputest_tail.txt
cat $PROFILE_OUT/r06_gputest_tail.txt
