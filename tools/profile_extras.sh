#!/bin/bash
# The round-4 additions to a round's profile set, on the GPU box: bash tools/profile_extras.sh <tag>   (after tools/profile_round.sh <tag>)
# Copy what should be judged from $OUT_DIR/ into profiles/ afterwards.
tag=$1
out=${OUT_DIR:?set OUT_DIR to the folder that collects the results}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
# ---- round 4: the new entry points, each with its own small tool (JSON lines under $OUT_DIR/<tag>_*.json) ----
timeout -k 10 200 python3 tools/time_mixed.py --reps 200 2>/dev/null | tail -1 > $out/${tag}_mixed_vs_f32.json
timeout -k 10 200 python3 tools/time_two_streams.py 2>/dev/null | tail -1 > $out/${tag}_two_streams.json
timeout -k 10 200 python3 tools/time_sqdiff.py 2>/dev/null | tail -1 > $out/${tag}_dequant_inv_sqdiff.json
timeout -k 10 200 python3 tools/time_multi.py 2>/dev/null | tail -1 > $out/${tag}_fwd_quant_multi.json
timeout -k 10 200 python3 tools/time_voxmerge.py 2>/dev/null | tail -1 > $out/${tag}_voxelize_merge.json
timeout -k 10 300 python3 tools/e2e_frame.py --entropy gpu --keep-rec 0 --out $out/${tag}_e2e > $out/${tag}_e2e_frame_gpu_entropy.txt 2>&1
timeout -k 10 300 python3 tools/e2e_frame.py --entropy gpu --keep-rec 0 --batch-steps 1 --out $out/${tag}_e2e > $out/${tag}_e2e_frame_gpu_entropy_batched.txt 2>&1
timeout -k 10 200 python3 tools/time_rlgr_batch.py 3 2048 2>/dev/null | tail -1 > $out/${tag}_rlgr_batch.json
timeout -k 10 200 python3 tools/prelude_loop.py > $out/${tag}_prelude_wall.txt 2>/dev/null
timeout -k 10 300 bash tools/trace_mx.sh ${tag} > $out/${tag}_mixed_kernel_durations.txt 2>&1
timeout -k 10 400 bash tools/pmc_rlgr.sh ${tag} > $out/${tag}_rlgr_sq_counters.txt 2>&1
timeout -k 10 400 bash tools/pmc_rlgr.sh ${tag}_batch tools/time_rlgr_batch.py 2 > $out/${tag}_rlgr_batch_sq_counters.txt 2>&1
timeout -k 10 300 bash tools/pmc_mx.sh ${tag}mx > $out/${tag}_mixed_sq_counters.txt 2>&1
# N > 1 rehearsal on the one GPU (4 ranks: the process guard allows 6 processes on the card, and the launcher and the parent count), so that the multi_gpu fields of such a line can be reviewed
timeout -k 10 500 python3 bench.py --full --gpus 4 --backend gloo --workload cfg5 --rows 6000000 --steps 20 --warmup 5 --settle-steps 0 --skip-legs --skip-prelude > $out/${tag}_rehearsal_4rank_cfg5_gloo_one_gpu.json 2>> $out/${tag}_bench.err
for f in mixed_vs_f32 two_streams dequant_inv_sqdiff fwd_quant_multi voxelize_merge; do echo "$f: $(cat $out/${tag}_$f.json | cut -c1-400)"; done
