"""Per-step kernel times from a rocprofv3 --kernel-trace CSV of bench.py: the last N replayed steps (a step ends with
k_adam_steps), per kernel name the mean us per step and launches per step, as one JSON line.
  python scripts/trace_per_step.py TRACE.csv [--steps 60] [--tag NAME]"""
import argparse, collections, csv, json, re

ap = argparse.ArgumentParser()
ap.add_argument('trace')
ap.add_argument('--steps', type=int, default=60)
ap.add_argument('--tag', default='')
args = ap.parse_args()

rows = []
with open(args.trace, newline='') as f:
    for r in csv.DictReader(f):
        name = re.sub(r'\(.*$', '', r['Kernel_Name']).replace('void ', '').strip()
        rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), name))
rows.sort()
ends = [i for i, r in enumerate(rows) if r[2].startswith('k_adam_steps')]
assert len(ends) > args.steps + 1, 'only %d steps in the trace' % len(ends)
lo, hi = ends[-args.steps - 1] + 1, ends[-1] + 1
us, cnt = collections.Counter(), collections.Counter()
for s, e, name in rows[lo:hi]:
    us[name] += (e - s) / 1e3
    cnt[name] += 1
wide = {k: round(v / args.steps, 2) for k, v in us.items() if re.match(r'k_conv_fwd_u<(26|30|34),\s*16,\s*27>|k_conv_fwd_u<16,\s*(26|30|34),\s*27>', k)}
print(json.dumps({
    'tag': args.tag, 'steps': args.steps, 'launches_per_step': round((hi - lo) / args.steps, 2),
    'kernel_us_per_step': round(sum(us.values()) / args.steps, 1),
    'wall_us_per_step': round((rows[hi - 1][1] - rows[lo][0]) / 1e3 / args.steps, 1),
    'wide_conv_us_per_step': wide, 'wide_conv_sum_us': round(sum(wide.values()), 2),
    'kernels': {k: [round(v / args.steps, 2), round(cnt[k] / args.steps, 2)] for k, v in us.most_common()}}))
