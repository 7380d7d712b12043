set -o pipefail
O=${O:-ab_out}
mkdir -p $O
for r in 1 2 3; do for pw in 1 2 3; do
timeout -k 10 120 python bench.py --config easy --full --no-cpu-baseline --no-roofline --prewarm-s $pw > $O/pw.log 2>&1 || exit 1
python3 -c "
import json,sys
d=json.loads([l for l in open(sys.argv[2]) if l.startswith('{')][-1])
print('prewarm', sys.argv[1], round(d['value']/1e6,1), 'M', d['ms_per_step'], d['train_stats']['prewarm'])" $pw $O/pw.log
done; done
