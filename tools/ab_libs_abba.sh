#!/bin/bash
# Same-box A/B of two builds of libdm_engine.so on the graded bench step in ABBA order (see tools/ab_option.sh for why):
#     bash tools/ab_libs_abba.sh <libA.so> <libB.so> [quads=2] [steps=8]
# Every bench run has its own time limit (BENCH_TIMEOUT seconds, default 300) and the first run that fails ends the series: nothing
# more is started on a device a run has just faulted or hung.  The summary gives, per arm, the mean and the spread between its
# repeats (max - min and the standard deviation): a difference counts only from twice that spread up.
A=$1; B=$2; QUADS=${3:-2}; STEPS=${4:-8}
line() { python -c "import json,sys; d=json.loads(sys.stdin.read()); print('%9.3f ms/step %8.4f img/s  igemm %7.2f TF/s (%6.2f ms)  attn %6.2f TF/s  checksum %r' % (d['ms_per_step'], d['value'], d['roofline']['achieved'], d['roofline']['kernel_ms_total']/d['steps'], d['roofline']['attention_tflops'], d['scores_checksum']))"; }
run() {
    echo -n "$1 $(basename $2): "
    out=$(DM_ENGINE_LIB=$2 timeout -k 10 ${BENCH_TIMEOUT:-300} python bench.py --steps $STEPS --warmup 2 --no-cpu-baseline --no-side --no-parity 2>/dev/null)
    rc=$?
    if [ $rc -ne 0 ]; then echo "bench.py failed, exit status $rc: series ended"; return 1; fi
    echo "$out" | line
}
for i in $(seq $QUADS); do run A $A && run B $B && run B $B && run A $A || break; done | tee /tmp/ab_libs.$$
python - <<PY
import re
a, b = [], []
for l in open('/tmp/ab_libs.$$'):
    m = re.match(r'([AB]) \S+:\s+([\d.]+) ms/step', l)
    if m: (a if m.group(1) == 'A' else b).append(float(m.group(2)))
def sd(v):
    m = sum(v) / len(v)
    return (sum((x - m) ** 2 for x in v) / max(1, len(v) - 1)) ** 0.5
if a and b:
    ma, mb = sum(a) / len(a), sum(b) / len(b)
    print('mean A %.3f ms/step (n=%d)   B %.3f ms/step (n=%d)   B - A %+.3f ms' % (ma, len(a), mb, len(b), mb - ma))
    spread = max(max(a) - min(a), max(b) - min(b))
    print('spread between repeats of one arm: A max-min %.3f (sd %.3f)   B max-min %.3f (sd %.3f)   |B - A| / larger spread = %.2f'
          % (max(a) - min(a), sd(a), max(b) - min(b), sd(b), abs(mb - ma) / spread if spread > 0 else float('inf')))
PY
rm -f /tmp/ab_libs.$$
