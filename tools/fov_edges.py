"""The sweep behind tests/fov_edges.py: every odd FoV (zyx) up to --max per axis and --max-x
along x with V <= --max-v through the rules of conv_caps (ffn_amd/csrc/ffn_stack_plan.h),
restated here in numpy -- no GPU, no header.  Per limit of the rules it prints the
geometries with the least slack on either side (smallest V first), then the census of
(default_variant, oa) and what chose each row of kPerms.

  python tools/fov_edges.py                       # 3 .. 65 per axis, V <= 70,000
  python tools/fov_edges.py --max 131 --max-x 131 # up to the widest row conv32 stages
  python tools/fov_edges.py --check 300           # closed-form spans against brute force

Span of a chunk: dense order is monotone in the padded position z plane + y XS + x, so a
chunk's span is pad(last) - pad(first) + 1; the largest over the chunks is what a kernel
must stage.  The constants are the ones tests/test_stack_plan.py restates; depth >= 2.
"""
import argparse
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from tests.test_stack_plan import (C_CHUNK, D_CHUNK, E_CHUNK, E_ROWS, H_CHUNK, H_ROWS,  # noqa: E402
                                   M_CHUNK, M_ROWS, T3_ROWS, T_ROWS, _span)

PERMS = [(0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]  # the header's order
RCK_MAX, TAIL_MAX, MAIN, LDS_MAX = 320, 256, 256, 160 * 1024


def span(f, chunk, start=0):
  """largest padded span of the chunks of `chunk` dense voxels from dense voxel `start`"""
  fz, fy, fx = f
  v = fz * fy * fx
  lo = np.arange(start, v, chunk, dtype=np.int64)
  hi = np.minimum(lo + chunk, v) - 1

  def pad(d):
    return (d // (fx * fy)) * ((fy + 1) * (fx + 1)) + ((d // fx) % fy) * (fx + 1) + d % fx

  return int((pad(hi) - pad(lo)).max()) + 1


def rules(fov):
  """conv_caps of one FoV at depth >= 2: its flags, and `slack`: limit -> budget - need
  (negative: the geometry misses that limit)"""
  v = fov[0] * fov[1] * fov[2]

  def m_need(f):
    return span(f, M_CHUNK) + 2 * (f[2] + 2)

  oa, fits = (0, 1, 2), []
  if m_need(fov) > M_ROWS:
    fits = [p for p in PERMS if m_need(tuple(fov[a] for a in p)) <= M_ROWS]
    if fits:
      oa = min(fits, key=lambda p: fov[p[2]])  # the first of the shortest rows
  q = tuple(fov[a] for a in oa)
  halo = 2 * (q[2] + 2)
  r = {'fov': fov, 'V': v, 'oa': oa, 'fits': fits, 'slack': {}}
  s = r['slack']
  rc = max(256, (span(fov, C_CHUNK) + 2 * (fov[2] + 2) + 31) // 32 * 32)
  rck_raw = span(q, D_CHUNK) + halo
  rck = max(256, (rck_raw + 31) // 32 * 32)
  nk, ne, nm = -(-v // D_CHUNK), -(-v // E_CHUNK), -(-v // M_CHUNK)
  r.update(Rc=rc, Rc_k=rck, rck_raw=rck_raw, nchunks_m=nm, nchunks_k=nk)
  s['lds_bytes <= 160 KB'] = (LDS_MAX - 3 * (160 + 2 * (fov[2] + 2)) * 128) // 768  # in voxels of fx
  s['Rc_k <= 320'] = RCK_MAX - rck
  s['Rc_k raw <= 320'] = RCK_MAX - rck_raw
  d_ok = rck <= RCK_MAX and nk >= 2
  s['kERows'] = E_ROWS - (span(q, E_CHUNK) + halo)
  s['kMRows'] = M_ROWS - (span(q, M_CHUNK) + halo)
  e_ok = d_ok and s['kERows'] >= 0 and ne >= 2
  m_ok = d_ok and s['kMRows'] >= 0 and nm >= 2
  t_ok = False
  r.update(n_tail=0, n_tail3=0, tail_voxels=0)
  if m_ok:
    s['nchunks_m <= 256'] = MAIN - nm
  if m_ok and nm > MAIN:
    rest = v - MAIN * M_CHUNK
    n_tail = -(-rest // 32)
    r.update(n_tail=n_tail, n_tail3=-(-rest // 96), tail_voxels=rest - (n_tail - 1) * 32)
    s['kTRows'] = T_ROWS - (span(q, 32, MAIN * M_CHUNK) + halo)
    s['kT3Rows'] = T3_ROWS - (span(q, 96, MAIN * M_CHUNK) + halo)
    s['n_tail <= 256'] = TAIL_MAX - n_tail
    t_ok = s['kTRows'] >= 0 and s['kT3Rows'] >= 0 and n_tail <= TAIL_MAX
  if t_ok:
    s['kHRows'] = H_ROWS - (span(q, H_CHUNK) + halo)
  exact = 2 if rc in (256, 288) else 0
  r.update(d_ok=d_ok, e_ok=e_ok, m_ok=m_ok, t_ok=t_ok, exact=exact,
           h_geom_ok=t_ok and s['kHRows'] >= 0,
           default=9 if t_ok else 8 if m_ok else 6 if d_ok else exact)
  return r


def geometries(max_zy, max_x, max_v):
  for fz in range(3, max_zy + 1, 2):
    for fy in range(3, max_zy + 1, 2):
      if fz * fy * 3 > max_v:
        break
      for fx in range(3, max_x + 1, 2):
        if fz * fy * fx > max_v:
          break
        yield (fz, fy, fx)


def line(r, limit):
  return '    %-14s V %6d  slack %4d  default %d exact %d oa %s Rc_k %d (raw %d) n_tail %d' % (
      'x'.join(str(f) for f in r['fov']), r['V'], r['slack'][limit], r['default'], r['exact'],
      r['oa'], r['Rc_k'], r['rck_raw'], r['n_tail'])


def main():
  ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
  ap.add_argument('--max', type=int, default=65, help='largest fz, fy')
  ap.add_argument('--max-x', type=int, default=0, help='largest fx (default: --max)')
  ap.add_argument('--max-v', type=int, default=70000)
  ap.add_argument('--show', type=int, default=3, help='geometries per limit and side')
  ap.add_argument('--check', type=int, default=0,
                  help='compare span() with the brute force of tests/test_stack_plan.py '
                       'on this many random geometries, then exit')
  args = ap.parse_args()
  if args.check:
    rng = np.random.RandomState(0)
    for _ in range(args.check):
      f = tuple(int(x) for x in rng.randint(1, 20, 3) * 2 + 1)
      chunk = int(rng.choice([32, 80, 96, 128, 144, 160]))
      start = int(rng.choice([0, min(MAIN * M_CHUNK, (f[0] * f[1] * f[2] - 1) // 32 * 32)]))
      assert span(f, chunk, start) == _span(f, chunk, start), (f, chunk, start)
    print('span() == brute force on %d geometries' % args.check)
    return
  max_x = args.max_x or args.max
  all_r = [rules(f) for f in geometries(args.max, max_x, args.max_v)]
  all_r = [r for r in all_r if r['slack']['lds_bytes <= 160 KB'] >= 0]  # the engine takes it
  print('%d geometries: odd fz, fy in 3 .. %d, fx in 3 .. %d, V <= %d, rows conv32 can stage'
        % (len(all_r), args.max, max_x, args.max_v))
  limits = ['kMRows', 'kERows', 'Rc_k raw <= 320', 'kTRows', 'kT3Rows', 'kHRows',
            'n_tail <= 256', 'nchunks_m <= 256', 'lds_bytes <= 160 KB']
  for limit in limits:
    have = [r for r in all_r if limit in r['slack']]
    print('\n%s  (%d geometries reach this rule)' % (limit, len(have)))
    for side, sel, key in (
        ('inside', [r for r in have if r['slack'][limit] >= 0],
         lambda r: (r['slack'][limit], r['V'])),
        ('missed', [r for r in have if r['slack'][limit] < 0],
         lambda r: (-r['slack'][limit], r['V']))):
      print('  %s, least slack first:' % side)
      for r in sorted(sel, key=key)[:args.show]:
        print(line(r, limit))
  print('\nextremes among default 9:')
  nine = [r for r in all_r if r['default'] == 9]
  for what, key in (('fewest tail voxels', lambda r: (r['n_tail'], r['tail_voxels'], r['V'])),
                    ('most tail workgroups', lambda r: (-r['n_tail'], r['V']))):
    for r in sorted(nine, key=key)[:args.show]:
      print('  %-22s %-14s V %6d n_tail %3d (last %2d voxels) n_tail3 %3d oa %s exact %d' % (
          what, 'x'.join(str(f) for f in r['fov']), r['V'], r['n_tail'], r['tail_voxels'],
          r['n_tail3'], r['oa'], r['exact']))
  print('\ncensus of (default_variant, oa):')
  census = collections.Counter((r['default'], r['oa']) for r in all_r)
  for (default, oa), count in sorted(census.items()):
    first = min((r for r in all_r if (r['default'], r['oa']) == (default, oa)),
                key=lambda r: r['V'])
    print('  default %d oa %s: %6d  (%.1f %%)  smallest %s' % (
        default, oa, count, 100.0 * count / len(all_r), 'x'.join(str(f) for f in first['fov'])))
  print('\nrows of kPerms:')
  for p in PERMS:
    chose = [r for r in all_r if r['oa'] == p]
    fit = [r for r in all_r if p in r['fits']]
    if chose:
      first = min(chose, key=lambda r: r['V'])
      print('  %s chosen by %d geometries, smallest %s' % (
          p, len(chose), 'x'.join(str(f) for f in first['fov'])))
    else:
      print('  %s chosen by NO geometry (it fits %d; each of them chose a row with shorter '
            'rows, or an earlier one with rows as short)' % (p, len(fit)))


if __name__ == '__main__':
  main()
