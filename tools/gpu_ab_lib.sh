# Interleaved short benches of two builds of the working tree: the default libavr.so and an
# experiment library (LIB, e.g. assistive-vr-gym_amd/avr/libavr_fuse.so via AVR_LIB), ROUNDS times
# each, task TASK.  Timing only.
set -o pipefail
cd /root/repo && export TMPDIR=/tmp && mkdir -p gpurun_out/abl
T=${TASK:-FeedingJaco-v0}
O=${AB_OUT:-$(mktemp -d)} && mkdir -p $O      # bench lines and their stderr; the summary is printed
for r in $(seq 1 ${ROUNDS:-2}); do
  for tag in base exp; do
    if [ $tag = exp ]; then export AVR_LIB=$LIB; else unset AVR_LIB; fi
    timeout -k 10 200 python3 bench.py --task $T --steps 30 --warmup 3 --no-cpu-baseline --other-steps 0 > $O/b_${tag}_$r.json 2> $O/b_${tag}_$r.err || exit $?
    echo $T $tag $r $(python3 -c "import json;d=json.loads(open('$O/b_${tag}_$r.json').read().strip().splitlines()[-1]);print(round(d['value']), d['nan_or_overflow_envs'])")
  done
done
unset AVR_LIB
