#!/usr/bin/env python3
"""Wall clock, kernel time and GPU idle of one complete segment_all pass, from a
rocprofv3 --kernel-trace CSV of bench.py (no counters in that run).

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o s -- python bench.py ...
  python tools/pass_idle.py DIR/.../s_kernel_trace.csv [--gap-ms 10] [--list]

The launches are cut into stretches wherever the GPU stood idle for more than --gap-ms
(a volume read back: nothing inside a pass comes near) and at every device memset (a
canvas being made: bench.py makes a new one for the pass, 3 ms behind the timed leg).
The stretch with the most FoV stacks is the complete pass: 24 k steps against the 4 k of
the timed leg.  For it: wall clock (first start to last end), the sum of the kernel
durations, the time at least one kernel was running (launches made ahead overlap the
step before them, so the sum counts some time twice), their difference = GPU idle, and
the number of between-segment turns (turn_publish_kernel, one per turn)."""
import argparse
import csv


def stretches(rows, gap_ns):
  out, end = [[]], None
  for r in rows:
    if 'fillBuffer' in r[2]:  # hipMemset: belongs to neither side
      end = None
      continue
    if end is None or r[0] - end > gap_ns:
      out.append([])
      end = r[1]
    out[-1].append(r)
    end = max(end, r[1])
  return [p for p in out if p]


def summary(rows):
  wall = max(r[1] for r in rows) - rows[0][0]
  total = sum(r[1] - r[0] for r in rows)
  busy, end = 0, rows[0][0]
  for s, e, _ in rows:
    if e > end:
      busy += e - max(s, end)
      end = e
  count = lambda key: sum(1 for r in rows if key in r[2])
  return {'launches': len(rows), 'stacks': count('conv32'), 'turns': count('turn_publish'),
          'wall_ms': wall / 1e6, 'kernel_sum_ms': total / 1e6, 'busy_ms': busy / 1e6,
          'idle_ms': (wall - busy) / 1e6}


def main():
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('trace')
  ap.add_argument('--gap-ms', type=float, default=10.0)
  ap.add_argument('--list', action='store_true', help='every stretch of 1000+ launches')
  args = ap.parse_args()
  rows = []
  with open(args.trace) as f:
    for r in csv.DictReader(f):
      rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']))
  rows.sort()
  parts = [summary(p) for p in stretches(rows, args.gap_ms * 1e6)]
  if args.list:
    for p in parts:
      if p['launches'] >= 1000:
        print('stretch: %(launches)d launches, %(stacks)d stacks, %(turns)d turns, '
              'wall %(wall_ms).1f ms, idle %(idle_ms).1f ms' % p)
  best = max(parts, key=lambda p: p['stacks'])
  print('complete pass: %(launches)d launches (%(stacks)d conv stacks, %(turns)d turns); '
        'wall %(wall_ms).1f ms, kernels %(kernel_sum_ms).1f ms summed / %(busy_ms).1f ms '
        'with at least one running; GPU idle %(idle_ms).1f ms' % best
        + ' (%.2f %% of the pass)' % (100.0 * best['idle_ms'] / best['wall_ms']))


if __name__ == '__main__':
  main()
