R=${GRAFT_REPO_ROOT:-/root/repo}
cd $R
O=${1:-build/hunt}
mkdir -p $O
python profiles/tools/gpu_sampler.py $O/r05_hunt_samples.txt & SP=$!
for i in 1 2 3; do
  IMPDAR_TRACE=1 python bench.py --full --no-e2e > $O/r05_hunt_$i.json 2> $O/r05_hunt_$i.err
  python - $i $O <<'PY'
import re, sys
i, o = sys.argv[1], sys.argv[2]
idle = None
for l in open('%s/r05_hunt_%s.err' % (o, i)):
    m = re.search(r'unix ([0-9.]+)\] ps_runs: (stream idle|ps_runs_kernel done)', l)
    if not m: continue
    t = float(m.group(1))
    if m.group(2) == 'stream idle': idle = t
    elif idle is not None:
        print('run', i, 'ps_runs_kernel %.1f ms at unix %.3f' % ((t - idle) * 1e3, idle))
        if (t - idle) > 0.03:
            rows = [r for r in open('%s/r05_hunt_samples.txt' % o) if idle - 0.15 < float(r.split()[0]) < t + 0.1]
            print(''.join(rows[:40]))
PY
done
kill $SP
