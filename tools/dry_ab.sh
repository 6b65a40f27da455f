# Micro-steps per iteration once a wave's queue is dry (SAHARA_TEXT_STEPS_DRY),
# in-process A/Bs; C2's bench line; the CLI at C3 scale (index load through the ring).
mkdir -p gpurun_out
timeout -k 10 500 python3 tools/ab_inproc.py --rounds 3 --steps 10 --count d0= d4=SAHARA_TEXT_STEPS_DRY=4 d8=SAHARA_TEXT_STEPS_DRY=8 d16=SAHARA_TEXT_STEPS_DRY=16 > gpurun_out/dry_dr.txt 2>&1 || exit 1
timeout -k 10 500 python3 tools/ab_inproc.py --rounds 3 --steps 10 --packed d0= d4=SAHARA_TEXT_STEPS_DRY=4 d8=SAHARA_TEXT_STEPS_DRY=8 d16=SAHARA_TEXT_STEPS_DRY=16 > gpurun_out/dry_packed.txt 2>&1 || exit 1
tail -5 gpurun_out/dry_dr.txt; tail -5 gpurun_out/dry_packed.txt
C2=$(mktemp -d) || exit 1
timeout -k 10 300 python3 bench.py --full --config c2 --no-cpu > $C2/c2.json 2> $C2/c2.err || exit 1
python3 -c "import json; d=json.load(open('$C2/c2.json')); print('c2', d['value'], d['ms_per_step'], d['config']['device_resident']['reads_per_s'])"
bash tools/cli_scale.sh gpurun_out/r6_cli_scale || exit 1
tail -12 gpurun_out/r6_cli_scale/search.txt; cat gpurun_out/r6_cli_scale/search.err | grep sahara | head
