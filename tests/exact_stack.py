"""Conv stacks on which every conv kernel of the engine must return the f64 oracle's bits:
the models, inputs and preconditions that tests/test_exact_stack.py (CPU) and
tests/test_gpu_exact_stack.py (GPU) share.  Not a test.

Why no tolerance is needed.  Let every operand of a conv (activations, weights, bias, the
residual-stream value added behind it) be a multiple of one power of two g, the conv's
grid, and let  S = sum |w| |x| + |b| + |x_residual|  of every output stay below 2^24 g.
Then every partial sum of the output's terms, in any association order, is a multiple of g
below 2^24 g in magnitude: an f32 value.  No addition ever rounds, so the f64 oracle, the
sequential-f32 oracle, the f32-MFMA kernels and any other order of the same terms give the
same bits, and a term that is dropped, doubled, misplaced or misweighted moves the output
by at least g.

The split-product kernels (conv_variant 6 .. 10) add one condition.  They carry an f32
value v as two fp16 numbers (split8_fp16 in ffn_amd/csrc/ffn_conv_split.h for activations,
split_fp16x2 in ffn_hip.hip's set_weights for weights):

  hi  = fp16(v), round to nearest even, 11 significant bits (0 where |v| < 2^-14)
  res = fp16((v - hi) 2048)

 * v - hi is computed in f32 and is exact (Sterbenz; below 2^-14 it is v itself).  For a v
   of at most 22 significant bits inside the fp16 range (|v| <= 65504), v - hi has at most
   11 significant bits and lies at or below half an ulp of hi, 2^-11 |v|; times 2048 it is
   below |v| and above 2^-14 2^-11 2^11 = 2^-14 unless v is below 2^-14 altogether, where
   hi = 0 and res = 2048 v >= 2^-14 still (the grids used here are 1 and 2^-11): res is a
   normal fp16 number, exact, and hi + res / 2048 == v.
 * An fp16 x fp16 product has at most 22 significant bits: exact in f32.  The MFMA
   accumulators are f32: two per output, acc for hi x hi and accC for the cross products
   hi_w res_x and res_w hi_x, joined as acc + 2^-11 accC.  Every term of acc is a multiple
   of g (hi of a multiple of g is one: rounding a multiple of g to fewer bits gives a
   multiple of g), every term of accC a multiple of 2048 g, and
   sum |hi_w| |res_x| <= 2048 2^-11 sum |w| |x|: both accumulators and their join stay
   below the same 2^24 g, hence exact.
 * res_w res_x is NOT computed.  A conv is therefore exact only if one side has no
   residual at all: every activation it reads, or every weight, is an fp16 value (at most
   11 significant bits, not below 2^-14).
 * A |value| above 65504 anywhere voids the step and repeats it on exact_variant (the
   range guard, range_max > 0x477fe000): the test would then check the wrong kernel.  The
   preconditions keep every operand and pre-activation at or below 32768, and every GPU
   test asserts afterwards that conv_variant is what it set.
 * With engine option mfma_products = 1 only hi x hi is computed: exact if BOTH sides are
   fp16 values (preconditions(..., one_product=True)).

conv0_a (2 -> 32) and the head (conv_lom, seed + update) are plain f32 in every kernel: the
grid argument alone covers them; the head's bound is 2^24 grid units.

preconditions() measures all of this on the f64 forward pass and raises if a case misses
one of the caps.  The caps bound the INPUTS of the test (half the hard limits: 2^23 grid
units for the sums, 32768 for the values); they are no tolerance on a kernel.  If a case
misses one, the case is changed, never the cap."""

import collections

import numpy as np

from tests import fov_edges
from tests import half_ref

FP16_BITS = 11          # significant bits of an fp16 value
SPLIT_BITS = 22         # of hi + res / 2048
VALUE_CAP = 32768.0     # operands and pre-activations (the range guard sits at 65504)
SUM_CAP = 2.0 ** 23     # sum of the |terms| of an output, in grid units (hard limit 2^24)
HEAD_CAP = 2.0 ** 24    # the head's sum, in grid units
WRES = 1.0 + 2.0 ** -11  # a weight of 12 significant bits: hi = 1, res = 1

SIGNS = (1.0, -1.0, 1.0, -1.0, 1.0, -1.0)
DENSE_GRID = 0.25


def conv_names(depth):
  names = ['conv0_a', 'conv0_b']
  for i in range(1, depth):
    names += ['conv%d_a' % i, 'conv%d_b' % i]
  return names


def _key(name, what):
  return 'seed_update/%s/%s' % (name, what)


def _sparse_conv(rng, cin, nz):
  """[3, 3, 3, cin, 32] with nz weights +1, -1, +1, ... per output channel.  cin 32: placed
  by nz channel permutations, so every input channel is read nz times, each at a random
  tap.  cin 2: a random (tap, channel) each.  No two land on the same entry."""
  w = np.zeros((27, cin, 32), np.float32)
  for k in range(nz):
    chan = rng.permutation(32) if cin == 32 else rng.randint(0, cin, 32)
    for co in range(32):
      while True:
        tap = rng.randint(27)
        if w[tap, chan[co], co] == 0:
          break
        if cin != 32:
          chan[co] = rng.randint(0, cin)
      w[tap, chan[co], co] = SIGNS[k]
  return w.reshape(3, 3, 3, cin, 32)


def _finish(rng, variables, depth, grid=1.0):
  """biases of -2 .. 2 grid units for every conv, and the +-1 head"""
  for name in conv_names(depth):
    variables[_key(name, 'biases')] = (rng.randint(-2, 3, 32) * grid).astype(np.float32)
  variables[_key('conv_lom', 'weights')] = (
      rng.randint(0, 2, (1, 1, 1, 32, 1)) * 2 - 1).astype(np.float32)
  variables[_key('conv_lom', 'biases')] = rng.randint(-2, 3, 1).astype(np.float32)
  return variables


def deep_sparse(depth, nz, seed):
  """Every conv gives each output channel nz weights +1, -1, ...; conv_lom is +-1."""
  rng = np.random.RandomState(seed)
  v = {}
  for name in conv_names(depth):
    v[_key(name, 'weights')] = _sparse_conv(rng, 2 if name == 'conv0_a' else 32, nz)
  return _finish(rng, v, depth)


def dense_shallow(seed, nz0=2):
  """Depth 2; all 864 weights of every output channel of the three 32 -> 32 convs are +-1:
  every tap x cin x cout entry of the kernels' weight fragments takes part.  Each conv
  multiplies the typical magnitude by sqrt(864) ~ 29: with integer inputs, even in
  [-1, 1], and integer biases conv1_b's pre-activation, the largest value of the stack,
  reaches 62,000.  So conv0_a is sparse (nz0 per output channel) and the whole case lives
  on the grid DENSE_GRID = 2^-2 -- the biases here, image and seed in exact_inputs are
  -2 .. 2 quarters (DENSE_AMP) -- which is an integer case scaled by a power of two: the
  same bits in every mantissa, values a quarter as large (15,800 at the most over the
  FoVs of CASES, a factor of 2 inside VALUE_CAP), sums in grid units unchanged.  conv1_b
  reads activations of 12 significant bits, so the residual planes are not idle either."""
  rng = np.random.RandomState(seed)
  v = {_key('conv0_a', 'weights'): _sparse_conv(rng, 2, nz0)}
  for name in conv_names(2)[1:]:
    # 432 of each sign per output channel, shuffled: its inputs are ReLU outputs, all
    # positive, and a channel with more of one sign would be negative (dead behind the
    # next ReLU) or positive almost everywhere
    w = np.stack([rng.permutation(np.repeat([1.0, -1.0], 432)) for _ in range(32)], axis=1)
    v[_key(name, 'weights')] = w.reshape(3, 3, 3, 32, 32).astype(np.float32)
  return _finish(rng, v, 2, DENSE_GRID)


def weight_residual(which, seed):
  """deep_sparse(2, 4, seed) in which the conv `which` (conv0_b, conv1_a or conv1_b)
  carries +-(1 + 2^-11): 12 significant bits, so its residual weight plane -- all zero
  under +-1 weights -- holds +-1.  Its inputs are integers of at most 11 bits (checked by
  preconditions: no conv with residuals on both sides), its outputs multiples of 2^-11;
  the later convs keep +-1 and only pass the finer grid on."""
  assert which in ('conv0_b', 'conv1_a', 'conv1_b')
  v = deep_sparse(2, 4, seed)
  v[_key(which, 'weights')] = (v[_key(which, 'weights')] * np.float32(WRES)).astype(
      np.float32)
  return v


def both_residuals(seed):
  """The control that must FAIL the preconditions: residual weights on conv0_b and on
  conv1_a, whose inputs (conv0_b's outputs, m (1 + 2^-11) + b) then carry residuals too."""
  v = weight_residual('conv0_b', seed)
  v[_key('conv1_a', 'weights')] = (v[_key('conv1_a', 'weights')] * np.float32(WRES)).astype(
      np.float32)
  return v


BUILDERS = dict(deep_sparse=deep_sparse, dense_shallow=dense_shallow,
                weight_residual=weight_residual, both_residuals=both_residuals)


def exact_inputs(n, fov_zyx, seed, amp=4, grid=1.0):
  """image and seed logits of -amp .. amp grid units (integers by default),
  [n, z, y, x] f32"""
  rng = np.random.RandomState(seed)
  shape = (n,) + tuple(fov_zyx)
  return ((rng.randint(-amp, amp + 1, shape) * grid).astype(np.float32),
          (rng.randint(-amp, amp + 1, shape) * grid).astype(np.float32))


# ---------------------------------------------------------------------------
# measuring a case
# ---------------------------------------------------------------------------


def bits_and_grid(*arrays):
  """(the largest number of significant bits -- first to last set bit of the mantissa --
  among the values of the arrays, the largest power of two that divides every value);
  zeros count for nothing: (0, 1.0) if there is nothing else.  The grid is never reported
  above 1.0 (integers are on the grid 1)."""
  import torch  # (several threads: the arrays of a 33^3 batch have millions of values)
  bits, low_exp = 0, 0
  for a in arrays:
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).reshape(-1)
    mant, exp = torch.frexp(t)  # a = mant 2^exp, 0.5 <= |mant| < 1
    # the 53-bit mantissa as an integer; bit 53 on top, so that a zero counts as a value
    # without significant bits on the grid 1 and no value has to be left out
    m = (mant.abs() * 2.0 ** 53).to(torch.int64) | (1 << 53)
    zeros = torch.log2((m & -m).double()).to(torch.int64)  # trailing zero bits
    bits = max(bits, 53 - int(zeros.min()))
    low_exp = min(low_exp, int((exp.long() - 53 + zeros).min()))  # of the last set bit
  return bits, 2.0 ** low_exp


def significant_bits(*arrays):
  return bits_and_grid(*arrays)[0]


def grid_of(*arrays):
  return bits_and_grid(*arrays)[1]


def has_tiny(a):
  """is some nonzero |value| below 2^-14, where the split puts everything in the residual"""
  a = np.abs(np.asarray(a, np.float64))
  return bool(np.any((a != 0) & (a < half_ref.TINY)))


def has_residual(a):
  """does split8_fp16 / split_fp16x2 leave a nonzero residual for some value of a"""
  a = np.asarray(a, np.float32)
  with np.errstate(over='ignore'):
    return bool(np.any(half_ref.hi_np(a) != a))


def trace(variables, depth, image, seed):
  """The f64 forward pass (torch), conv by conv: a list of dicts with name, x (the operand
  the conv reads, ReLU applied), w [3, 3, 3, cin, 32], b, skip (the residual-stream value
  added behind it, or None), pre (conv + b + skip) and abs_sum (sum |w| |x| + |b| +
  |skip|); then the head's (name 'head': x, w, b, seed, logits, abs_sum).  All numpy f64;
  activations are channel-first, [n, c, z, y, x] (channel_last() turns one around)."""
  import torch
  import torch.nn.functional as F
  image = np.asarray(image, np.float64)
  seed = np.asarray(seed, np.float64)
  if image.ndim == 3:
    image, seed = image[None], seed[None]

  def t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))

  def cl(a):
    return a.numpy()

  def sparse_conv(x, w, b):
    # one shifted plane per nonzero weight: the deep models have 128 per conv, and
    # torch's f64 conv3d would take seconds per FoV on them
    k = w.shape[0]
    pad = k // 2
    xp = F.pad(x, (pad,) * 6)
    n, _, fz, fy, fx = x.shape
    out = b.view(1, -1, 1, 1, 1).repeat(n, 1, fz, fy, fx)
    for kz, ky, kx, ci, co in zip(*np.nonzero(w)):
      out[:, co] += float(w[kz, ky, kx, ci, co]) * xp[:, ci, kz:kz + fz, ky:ky + fy,
                                                      kx:kx + fx]
    return out

  def conv(x, name):
    w = np.asarray(variables[_key(name, 'weights')], np.float64)
    b = t(variables[_key(name, 'biases')])
    if np.count_nonzero(w) <= 1024:
      return sparse_conv(x, w, b), sparse_conv(x.abs(), np.abs(w), b.abs())
    w = t(w).permute(4, 3, 0, 1, 2).contiguous()
    pad = w.shape[-1] // 2
    return F.conv3d(x, w, b, padding=pad), F.conv3d(x.abs(), w.abs(), b.abs(), padding=pad)

  out = []

  def record(name, x, skip):
    pre, s = conv(x, name)
    if skip is not None:
      pre, s = pre + skip, s + skip.abs()
    out.append(dict(name=name, x=cl(x), w=np.asarray(variables[_key(name, 'weights')],
                                                      np.float64),
                    b=np.asarray(variables[_key(name, 'biases')], np.float64),
                    skip=None if skip is None else cl(skip), pre=cl(pre), abs_sum=cl(s)))
    return pre

  with torch.no_grad():
    x = torch.stack([t(image), t(seed)], dim=1)
    net = record('conv0_b', torch.relu(record('conv0_a', x, None)), None)
    for i in range(1, depth):
      skip = net
      net = torch.relu(record('conv%d_a' % i, torch.relu(net), None))
      net = record('conv%d_b' % i, net, skip)
    net = torch.relu(net)
    upd, s = conv(net, 'conv_lom')
    logits = t(seed) + upd[:, 0]
    out.append(dict(name='head', x=cl(net), w=np.asarray(variables[_key('conv_lom', 'weights')],
                                                         np.float64),
                    b=np.asarray(variables[_key('conv_lom', 'biases')], np.float64),
                    seed=seed, logits=logits.numpy(),
                    abs_sum=(s[:, 0] + t(seed).abs()).numpy()))
  return out


def channel_last(a):
  """[c, z, y, x] or [n, c, z, y, x] of trace() -> [..., z, y, x, c]"""
  return np.ascontiguousarray(np.moveaxis(a, -4, -1))


Row = collections.namedtuple('Row', [
    'name', 'grid', 'max_operand', 'operand_bits', 'weight_bits', 'max_pre', 'max_stream',
    'abs_sum_units', 'x_residual', 'w_residual'])


def preconditions(variables, depth, image, seed, one_product=False, traced=None):
  """Measures the case on its f64 forward pass and returns one Row per conv and one for
  the head:

    grid           the power of two every term and every partial sum is a multiple of
    max_operand    the largest |activation| the conv reads
    operand_bits, weight_bits   the largest count of significant bits among them
    max_pre        the largest |conv + b (+ residual stream)|
    max_stream     the largest |residual-stream value| added behind the conv (0: none)
    abs_sum_units  the largest sum |w| |x| + |b| (+ |x_residual|), in units of grid
    x_residual, w_residual   does the fp16 split leave a residual on that side

  and raises ValueError unless, for every conv: operands, weights and pre-activations are
  at most VALUE_CAP = 32768 (half the fp16 range guard); they have at most SPLIT_BITS = 22
  significant bits (hi + res / 2048 is the value); abs_sum_units < SUM_CAP = 2^23 (half of
  2^24: every partial sum in every order is an f32 value); not both sides carry a residual
  (res x res is not computed); with one_product, neither side does (only hi x hi is
  computed).  The head: abs_sum_units < 2^24.  conv0_a is plain f32 in every kernel: its
  residual columns are reported and not judged.

  traced: the result of trace() on the same arguments, if the caller has it already.

  The caps are preconditions on the inputs, measured on the reference alone -- not a
  tolerance on a kernel.  A case that misses one is changed."""
  rows, faults = [], []

  def residual(a, bits, grid):  # the split leaves one: more than 11 bits, or below 2^-14
    return bits > FP16_BITS or (grid < half_ref.TINY and has_tiny(a))

  def largest(a):
    return max(float(a.max()), -float(a.min()))

  for c in traced or trace(variables, depth, image, seed):
    x_bits, x_grid = bits_and_grid(c['x'])
    w_bits, w_grid = bits_and_grid(c['w'])
    if c['name'] == 'head':
      g = min(x_grid * w_grid, grid_of(c['b'], c['seed']))
      units = float(c['abs_sum'].max()) / g
      rows.append(Row('head', g, largest(c['x']), x_bits, w_bits,
                      largest(c['logits']), largest(c['seed']),
                      units, False, False))
      if not units < HEAD_CAP:
        faults.append('head: sum of |terms| %.0f grid units >= 2^24' % units)
      continue
    skip = c['skip']
    g = min(x_grid * w_grid, grid_of(c['b']), 1.0 if skip is None else grid_of(skip))
    row = Row(c['name'], g, largest(c['x']), x_bits, w_bits,
              largest(c['pre']),
              0.0 if skip is None else largest(skip),
              float(c['abs_sum'].max()) / g, residual(c['x'], x_bits, x_grid),
              residual(c['w'], w_bits, w_grid))
    rows.append(row)
    biggest = max(row.max_operand, row.max_pre, row.max_stream,
                  largest(c['w']))
    if biggest > VALUE_CAP:
      faults.append('%s: |value| %.6g > %g' % (row.name, biggest, VALUE_CAP))
    if max(row.operand_bits, row.weight_bits) > SPLIT_BITS:
      faults.append('%s: %d significant bits > %d' % (
          row.name, max(row.operand_bits, row.weight_bits), SPLIT_BITS))
    if not row.abs_sum_units < SUM_CAP:
      faults.append('%s: sum of |terms| %.0f grid units >= 2^23' % (
          row.name, row.abs_sum_units))
    if row.name != 'conv0_a':
      if row.x_residual and row.w_residual:
        faults.append('%s: activations and weights both carry a split residual' % row.name)
      if one_product and (row.x_residual or row.w_residual):
        faults.append('%s: one product, but %s carry a split residual (%d / %d bits)' % (
            row.name, 'the activations' if row.x_residual else 'the weights',
            row.operand_bits, row.weight_bits))
  if faults:
    raise ValueError('not an exact case: ' + '; '.join(faults))
  return rows


def maxima(rows):
  """one line: the case's measured maxima over its convs (the head's sum apart)"""
  convs = [r for r in rows if r.name != 'head']
  head = rows[-1]
  return ('grid 2^%d, max |operand| %.6g (%d bits), max |pre| %.6g, max sum %.0f units '
          '(cap 2^23 = 8388608), head sum %.0f units' % (
              int(np.log2(min(r.grid for r in rows))), max(r.max_operand for r in convs),
              max(r.operand_bits for r in convs), max(r.max_pre for r in convs),
              max(r.abs_sum_units for r in convs), head.abs_sum_units))


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------

Case = collections.namedtuple('Case', [
    'name', 'builder', 'args', 'fov', 'deltas', 'depth', 'input_seed', 'n', 'amp', 'grid',
    'one_product'])


def _case(name, builder, args, fov, deltas, depth, input_seed, n, amp=4, grid=1.0,
          one_product=False):
  return Case(name, builder, tuple(args), tuple(fov), tuple(deltas), depth, input_seed, n,
              amp, grid, one_product)


FOV33 = ((33, 33, 33), (8, 8, 8))
CONFIGS4 = ((21, 41, 41), (5, 10, 10))  # zyx of the 41 x 41 x 21 (xyz) model, deltas 10, 10, 5
WHICH = ('conv0_b', 'conv1_a', 'conv1_b')
DENSE_AMP = 2  # image and seed range of the dense family, in units of DENSE_GRID


def _edge(name):
  e = fov_edges.BY_NAME[name]
  return e[1], e[2]


CASES = [
    # a / b: 33^3 at full depth, 4 nonzeros; n = 4 serves the batches
    _case('deep4_33', 'deep_sparse', (12, 4, 3), FOV33[0], FOV33[1], 12, 101, 4),
    # c: a batch of 17 where the oracle is cheap
    _case('deep4_last_one', 'deep_sparse', (12, 4, 3), *_edge('last_one'), 12, 102, 17),
    _case('deep4_perm021_small', 'deep_sparse', (12, 4, 3), *_edge('perm021_small'), 12, 103,
          17),
    # d: dense, every accepted variant
    _case('dense_33', 'dense_shallow', (5,), FOV33[0], FOV33[1], 2, 104, 1, DENSE_AMP, DENSE_GRID),
] + [
    _case('dense_' + e[0], 'dense_shallow', (5,), e[1], e[2], 2, 110 + k, 2, DENSE_AMP,
          DENSE_GRID)
    for k, e in enumerate(fov_edges.EDGES)
] + [
    # e: one conv with a residual weight plane
    _case('wres_%s_%s' % (which, tag), 'weight_residual', (which, 7), fov, deltas, 2,
          140 + k, 1)
    for k, (tag, (fov, deltas)) in enumerate(
        [('33', FOV33), ('perm021_resident', _edge('perm021_resident'))])
    for which in WHICH
] + [
    # f: the 41 x 41 x 21 model at depth 18, 2 nonzeros
    _case('deep2_configs4', 'deep_sparse', (18, 2, 9), CONFIGS4[0], CONFIGS4[1], 18, 150, 1),
    # g: one product: 2 nonzeros keep every operand an fp16 value; its control is deep4_33
    _case('deep2_33', 'deep_sparse', (12, 2, 9), FOV33[0], FOV33[1], 12, 151, 3,
          one_product=True),
]

BY_NAME = {c.name: c for c in CASES}


def build(case):
  """variables, image, seed of a case"""
  variables = BUILDERS[case.builder](*case.args)
  image, seed = exact_inputs(case.n, case.fov, case.input_seed, case.amp, case.grid)
  return variables, image, seed


# ---------------------------------------------------------------------------
# single-weight mutations
# ---------------------------------------------------------------------------


def mutate(variables, depth, rng):
  """A copy of the variables with one weight changed: a nonzero entry of a random conv
  (conv_lom included) zeroed, or 1 added to a random entry.  Returns (copy, description)."""
  names = conv_names(depth) + ['conv_lom']
  name = names[rng.randint(len(names))]
  out = {k: v for k, v in variables.items() if not k.startswith('__')}
  w = np.array(variables[_key(name, 'weights')], np.float32)
  flat = w.reshape(-1)
  if rng.randint(2):
    at = int(rng.choice(np.flatnonzero(flat)))
    what = 'zeroed'
    flat[at] = 0
  else:
    at = int(rng.randint(flat.size))
    what = 'plus 1'
    flat[at] += 1
  out[_key(name, 'weights')] = w
  return out, '%s %s at %s' % (name, what,
                               tuple(int(i) for i in np.unravel_index(at, w.shape)))


# ---------------------------------------------------------------------------
# the split and the three-product sum, restated on numpy
# ---------------------------------------------------------------------------


def split_np(v):
  """hi, res of split8_fp16 / split_fp16x2 as f32 arrays (res is the fp16 value stored:
  2048 times the part of v that hi leaves out)"""
  v = np.asarray(v, np.float32)
  hi = half_ref.hi_np(v)
  with np.errstate(over='ignore'):
    res = ((v - hi) * np.float32(2048)).astype(np.float16).astype(np.float32)
  return hi, res


def three_products(x, w, b, skip, order):
  """One 3x3x3 conv of one FoV as the split-product kernels define it -- acc = sum hi_w hi_x,
  accC = sum hi_w res_x + res_w hi_x, result (acc + 2^-11 accC) + b (+ skip); res_w res_x is
  left out -- with every product and every sum in f32, one term after the other.
  x [z, y, x, cin], w [3, 3, 3, cin, cout], skip [z, y, x, cout] or None.
  order 'tap': taps outermost, ascending;  'channel': input channels outermost, both
  descending, cross products swapped: a different association of the same terms."""
  f32 = np.float32
  xh, xr = split_np(x)
  wh, wr = split_np(w)
  fz, fy, fx, cin = xh.shape
  pad = ((1, 1), (1, 1), (1, 1), (0, 0))
  xh, xr = np.pad(xh, pad), np.pad(xr, pad)
  acc = np.zeros((fz, fy, fx, w.shape[-1]), f32)
  acc_c = np.zeros_like(acc)
  taps = [(kz, ky, kx) for kz in range(3) for ky in range(3) for kx in range(3)]
  if order == 'tap':
    terms = [(t, ci) for t in taps for ci in range(cin)]
  else:
    terms = [(t, ci) for ci in reversed(range(cin)) for t in reversed(taps)]
  for (kz, ky, kx), ci in terms:
    ah = xh[kz:kz + fz, ky:ky + fy, kx:kx + fx, ci, None]
    ar = xr[kz:kz + fz, ky:ky + fy, kx:kx + fx, ci, None]
    acc += ah * wh[kz, ky, kx, ci]
    if order == 'tap':
      acc_c += ar * wh[kz, ky, kx, ci]
      acc_c += ah * wr[kz, ky, kx, ci]
    else:
      acc_c += ah * wr[kz, ky, kx, ci]
      acc_c += ar * wh[kz, ky, kx, ci]
  assert acc.dtype == f32 and acc_c.dtype == f32
  out = (acc + acc_c * f32(2.0 ** -11)) + np.asarray(b, f32)
  if skip is not None:
    out = out + np.asarray(skip, f32)
  return out
