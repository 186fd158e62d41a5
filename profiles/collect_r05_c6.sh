#!/bin/bash
# round 5, after the MACS 3D kernels got their compile-time-sides instantiation (5 x 5): the full GPU suite, c6's profile
# set again, a MACS 3D parity sweep and the driver-like default line (run through gpurun)
R=$GRAFT_REPO_ROOT
cd $R
export PROFILE_OUT=${PROFILE_OUT:-$R/profile_out}; mkdir -p $PROFILE_OUT   # where every file of the session lands (git ignores the default)
(timeout 1500 python -m pytest tests -m gpu -q 2>&1 | tail -3) > $PROFILE_OUT/r05_gputest_tail.txt
bash $R/profiles/collect_profiles.sh r05 c6
cd $R
bash profiles/collect_sq.sh r05 c6 inst SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVES
STRESS_ONLY_MOD20=0,5,10,15 timeout 900 python scripts/stress_parity.py 1000 $PROFILE_OUT/r05_stress_macs3d.json > $PROFILE_OUT/r05_stress_macs3d.log 2>&1
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" >> $PROFILE_OUT/r05_gputest_tail.txt 2>&1
SECONDS=0
python bench.py --gpus 1 --steps 20 --warmup 5 --full > $PROFILE_OUT/r05_default_bench.json 2> $PROFILE_OUT/r05_default_bench.err
echo "default bench: $SECONDS s" >> $PROFILE_OUT/r05_gputest_tail.txt
cat $PROFILE_OUT/r05_gputest_tail.txt
tail -1 $PROFILE_OUT/r05_stress_macs3d.log | cut -c1-400
