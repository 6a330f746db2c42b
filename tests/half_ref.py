"""TEST INFRASTRUCTURE: the fp16 inference mode (engine option mfma_products = 1)
restated on torch-CPU, after oracle/ffn_oracle.forward_torch.

With the mode on, every 32 -> 32 conv computes  sum hi(w) * hi(a)  where hi() is the
f32 value rounded to nearest-even fp16 with |v| < 2^-14 becoming 0 -- what the engine
already stores as the hi half of its split operands (split8_fp16 for activations,
split_fp16x2 for weights).  Everything else is forward_torch's: conv0_a, the head
(conv_lom, seed + update), bias, ReLU, the residual add and the residual stream keep
the working precision.

  forward_half(..., acc='h64')  products and sums in f64 (operands still through hi()
                                of their f32 value): the mode's definition without any
                                rounding of its own
  forward_half(..., acc='h32')  products and sums in f32 (oneDNN's order): an
                                implementation of the definition as good as the GPU's;
                                its distance to h64 is the yardstick of the GPU tests
"""
import numpy as np

TINY = 2.0 ** -14  # the smallest normal fp16: what lies below goes to the residual half


def hi_np(v):
  """hi() of an f32 array, as f32."""
  v = np.asarray(v, np.float32)
  return np.where(np.abs(v) < TINY, np.float32(0), v).astype(np.float16).astype(np.float32)


def hi_variables(variables, depth):
  """The variables with hi() applied to the weights of every 32 -> 32 conv (conv0_b,
  conv<i>_a, conv<i>_b): what the mode multiplies with.  Biases, conv0_a and conv_lom
  stay as they are."""
  out = {k: v for k, v in variables.items() if not k.startswith('__')}
  names = ['conv0_b'] + ['conv%d_%s' % (i, ab) for i in range(1, depth) for ab in 'ab']
  for name in names:
    key = 'seed_update/%s/weights' % name
    out[key] = hi_np(variables[key])
  return out


def forward_half(image, seed, variables, depth, acc='h64', threads=None):
  """logits [n, z, y, x] (or [z, y, x]) f32 of the fp16 mode; acc: 'h64' or 'h32'."""
  import torch
  import torch.nn.functional as F
  assert acc in ('h64', 'h32')
  f64 = acc == 'h64'
  if threads:
    torch.set_num_threads(int(threads))
  image = np.asarray(image, np.float32)
  seed = np.asarray(seed, np.float32)
  squeeze = image.ndim == 3
  if squeeze:
    image, seed = image[None], seed[None]
  wide = torch.float64 if f64 else torch.float32

  def hi(t):  # the working precision -> f32 -> fp16 (RNE, tiny values flushed) -> back
    v = t.float()
    v = torch.where(v.abs() < TINY, torch.zeros_like(v), v)
    return v.half().to(wide)

  def wb(name, half):
    w = torch.from_numpy(np.ascontiguousarray(
        variables['seed_update/%s/weights' % name])).permute(4, 3, 0, 1, 2)
    b = torch.from_numpy(np.ascontiguousarray(variables['seed_update/%s/biases' % name]))
    w = hi(w) if half else w.to(wide)
    return w.contiguous(), b.to(wide)

  with torch.no_grad():
    s = torch.from_numpy(seed).to(wide)
    im = torch.from_numpy(image).to(wide)
    x = torch.stack([im, s], dim=1)
    net = torch.relu(F.conv3d(x, *wb('conv0_a', False), padding=1))
    net = F.conv3d(hi(net), *wb('conv0_b', True), padding=1)
    for i in range(1, depth):
      skip = net
      net = torch.relu(net)
      net = torch.relu(F.conv3d(hi(net), *wb('conv%d_a' % i, True), padding=1))
      net = F.conv3d(hi(net), *wb('conv%d_b' % i, True), padding=1) + skip
    net = torch.relu(net)
    out = s + F.conv3d(net, *wb('conv_lom', False))[:, 0]
  out = out.float().numpy()
  return out[0] if squeeze else out
