# Interleaved short benches: a previous tree (AB, default _ab2/: a git worktree with its libavr.so built) and the
# working tree, ROUNDS times each, task TASK (default FeedingJaco-v0).  Timing only.
set -o pipefail
cd /root/repo && export TMPDIR=/tmp && mkdir -p gpurun_out/abb
T=${TASK:-FeedingJaco-v0}
O=${AB_OUT:-$(mktemp -d)} && mkdir -p $O      # bench lines and their stderr; the summary is printed
for r in $(seq 1 ${ROUNDS:-2}); do
  for tree in ${AB:-_ab2} .; do
    tag=$([ $tree = . ] && echo new || echo old)
    extra="--other-steps 0"
    (cd $tree && timeout -k 10 200 python3 bench.py --task $T --steps 30 --warmup 3 --no-cpu-baseline $extra) > $O/b_${tag}_$r.json 2> $O/b_${tag}_$r.err || exit $?
    echo $T $tag $r $(python3 -c "import json;d=json.loads(open('$O/b_${tag}_$r.json').read().strip().splitlines()[-1]);print(round(d['value']), d['nan_or_overflow_envs'])")
  done
done
