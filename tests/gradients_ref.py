"""Oracle for the gradients unit (include/ffn_gradients.h,
ffn_amd/training/gradients.py): the conv stack of reference
convstack_3d.py:38-54 in torch on the CPU (F.conv3d, autograd), in f64 or f32.

Where a ReLU would stand it computes x * mask: with masks handed in, or x > 0
when none are given.  A gradient check that compares two independent forward
passes trips over the ReLU kink (one flipped sign in two million moves a
gradient by 2.4e-4 of its largest entry), so the GPU tests hand the GPU's own
masks to both the f64 and the f32 run here and check the masks separately.
The loss is the documented stable form of sigmoid cross entropy with logits,
weighted, as a mean over all voxels.
"""

import numpy as np
import torch
import torch.nn.functional as F


def conv_scopes(depth):
  names = ['conv0_a', 'conv0_b']
  for i in range(1, depth):
    names += ['conv%d_a' % i, 'conv%d_b' % i]
  names.append('conv_lom')
  return names


def random_variables(depth, seed=0, stddev=0.05, bias_stddev=0.05):
  """Variables with the checkpoint's names and shapes; biases are not zero."""
  rng = np.random.RandomState(seed)
  out = {}
  for name in conv_scopes(depth):
    shape = ((3, 3, 3, 2, 32) if name == 'conv0_a' else
             (1, 1, 1, 32, 1) if name == 'conv_lom' else (3, 3, 3, 32, 32))
    out['seed_update/%s/weights' % name] = rng.normal(
        0, stddev, shape).astype(np.float32)
    out['seed_update/%s/biases' % name] = rng.normal(
        0, bias_stddev, shape[-1:]).astype(np.float32)
  return out


def to_ncdhw(a, dtype):
  """[n, z, y, x, C] numpy -> [n, C, z, y, x] torch."""
  return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).permute(
      0, 4, 1, 2, 3).contiguous()


def to_ndhwc(t):
  return t.detach().permute(0, 2, 3, 4, 1).contiguous().numpy()


def conv(x, w, b=None):
  """x [n, C, z, y, x]; w in the checkpoint's [kz, ky, kx, cin, cout]."""
  k = w.shape[0]
  return F.conv3d(x, w.permute(4, 3, 0, 1, 2), b, padding=k // 2)


class _StableSoftplus(torch.autograd.Function):
  """max(x, 0) + log1p(exp(-|x|)) with its derivative sigmoid(x): autograd
  through clamp and abs would give 1 and 0 at x == 0, where the function is
  smooth and the derivative is 1 / 2."""

  @staticmethod
  def forward(ctx, x):
    ctx.save_for_backward(x)
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-torch.abs(x)))

  @staticmethod
  def backward(ctx, grad):
    x, = ctx.saved_tensors
    e = torch.exp(-torch.abs(x))
    return grad * torch.where(x >= 0, 1 / (1 + e), e / (1 + e))


def pixel_loss(logits, labels, weights):
  x, z = logits, labels
  return (weights * (_StableSoftplus.apply(x) - x * z)).mean()


def run(variables, depth, seed, image, labels, weights, dtype=torch.float64,
        masks=None, want_grads=True):
  """The whole stack.  seed, image, labels, weights: [n, z, y, x] numpy;
  masks: None or 2 * depth boolean arrays [n, z, y, x, 32] in network order.
  Returns a dict: loss (float), logits [n, z, y, x], grads {name: array in the
  checkpoint's shape}, pre (2 * depth arrays [n, z, y, x, 32])."""
  v = {k: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=want_grads)
       for k, a in variables.items()}
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
  seed_t, image_t, labels_t, weights_t = (t(seed), t(image), t(labels),
                                          t(weights))
  pre = []

  def relu(x):
    k = len(pre)
    pre.append(x)
    if masks is None:
      m = (x > 0).to(dtype)
    else:
      m = to_ncdhw(masks[k], dtype)
    return x * m

  W = lambda s: v['seed_update/%s/weights' % s]
  B = lambda s: v['seed_update/%s/biases' % s]
  net = conv(torch.stack([image_t, seed_t], dim=1), W('conv0_a'), B('conv0_a'))
  net = conv(relu(net), W('conv0_b'), B('conv0_b'))
  for i in range(1, depth):
    in_net = net
    net = conv(relu(net), W('conv%d_a' % i), B('conv%d_a' % i))
    net = conv(relu(net), W('conv%d_b' % i), B('conv%d_b' % i))
    net = net + in_net
  update = conv(relu(net), W('conv_lom'), B('conv_lom'))
  logits = seed_t + update[:, 0]
  loss = pixel_loss(logits, labels_t, weights_t)
  out = {'loss': float(loss.detach()), 'logits': logits.detach().numpy(),
         'pre': [to_ndhwc(p) for p in pre]}
  if want_grads:
    loss.backward()
    out['grads'] = {k: a.grad.numpy() for k, a in v.items()}
  return out


def conv_case(x, w, b, dy, relu_in=False, skip=None, dtype=torch.float64):
  """One conv with its three gradients by autograd.  x, dy, skip:
  [n, z, y, x, C] numpy (x may be a pair of [n, z, y, x] planes for cin 2).
  The ReLU mask is taken from x as given, so it is the same in f32 and f64.
  Returns y, dx (of conv(relu(x)) with respect to relu(x)), dW, db as numpy."""
  if isinstance(x, (tuple, list)):
    x = np.stack(x, axis=-1)
  if relu_in:
    x = np.maximum(x, 0)
  xt = to_ncdhw(x, dtype).requires_grad_(True)
  wt = torch.tensor(w, dtype=dtype, requires_grad=True)
  bt = torch.tensor(b, dtype=dtype, requires_grad=True)
  y = conv(xt, wt, bt)
  y.backward(to_ncdhw(dy, dtype))
  yv = to_ndhwc(y)
  if skip is not None:
    yv = yv + skip.astype(yv.dtype)
  return yv, to_ndhwc(xt.grad), wt.grad.numpy(), bt.grad.numpy()


def loss_case(logits, labels, weights, dtype=torch.float64):
  x = torch.tensor(logits, dtype=dtype, requires_grad=True)
  loss = pixel_loss(x, torch.tensor(labels, dtype=dtype),
                    torch.tensor(weights, dtype=dtype))
  loss.backward()
  return float(loss.detach()), x.grad.numpy()


def spread(g, g64):
  """E(g) = max |g - g_f64| / max |g_f64|."""
  g64 = np.asarray(g64, dtype=np.float64)
  return float(np.max(np.abs(np.asarray(g, dtype=np.float64) - g64)) /
               np.max(np.abs(g64)))


def training_inputs(n, zyx, seed=0):
  """A seeded normal image, seed logit(0.05) + N(0, 0.5) with logit(0.95) at
  the centre, labels 0.05 / 0.95, uniform weights; all [n, z, y, x] f32."""
  rng = np.random.RandomState(seed)
  shape = (n,) + tuple(zyx)
  logit = lambda p: np.log(p / (1 - p))
  image = rng.normal(0, 1, shape).astype(np.float32)
  s = (logit(0.05) + rng.normal(0, 0.5, shape)).astype(np.float32)
  s[:, zyx[0] // 2, zyx[1] // 2, zyx[2] // 2] = np.float32(logit(0.95))
  labels = np.where(rng.uniform(size=shape) < 0.3, 0.95, 0.05).astype(np.float32)
  weights = np.ones(shape, np.float32)
  return s, image, labels, weights
