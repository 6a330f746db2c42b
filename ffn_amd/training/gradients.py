"""Loss and gradients of ConvStack3DFFNModel on the GPU.

`GradientOps` is the handle over the gradients unit of libffn_hip.so
(include/ffn_gradients.h): conv forward, conv backward to the input, conv
backward to the weights, the 1x1x1 head and its gradient, and the weighted
pixelwise loss with its logit gradient, as device-to-device calls.

`ConvStackGradients` composes them into the whole stack (reference
convstack_3d.py:38-54, and backwards in reverse): for a batch of training FoVs
it returns the loss and its gradient with respect to every variable of the
model.  The contractions, reductions and the loss run in the unit only; torch
owns the device buffers and moves data, nothing else.  The parameter update
is trainer.ConvStackTrainer's, which hands this class its weight and gradient
storage and leaves the gradients on the device; there is no CPU fallback:
without a GPU the constructors raise.
"""

from __future__ import annotations

import ctypes
import threading

import numpy as np

from .. import _lib
from .. import _unit
from .._lib import check
from .models import convstack_3d

MAX_BATCH = 32
FEATURES = 32
#: what `last_timing` indexes
TIMED_CALLS = ('conv_forward', 'conv_backward_input', 'conv_backward_weights',
               'head_forward', 'head_backward', 'loss')


def _addr(a) -> int:
  """Address of a device array: an int, None (NULL) or an object with
  data_ptr()."""
  if a is None:
    return 0
  if hasattr(a, 'data_ptr'):
    return int(a.data_ptr())
  return int(a)


class GradientOps(_unit.Handle):
  """One stream + workspace for the gradient kernels.  Every argument that is
  an array is the address of dense f32 device memory (or an object with
  data_ptr()); `shape` is (z, y, x)."""

  def __init__(self, device_id: int = 0):
    super().__init__('ffn_gradients_create', 'ffn_gradients_destroy',
                     device_id)
    self.lock = threading.RLock()

  def conv_forward(self, n, shape, cin, x, x2, relu_in, w, b, skip, y):
    with self.lock:
      check(self._lib.ffn_gradients_conv_forward(
          self._h, int(n), _lib.i3(shape), int(cin), _addr(x), _addr(x2),
          int(bool(relu_in)), _addr(w), _addr(b), _addr(skip), _addr(y)))

  def conv_backward_input(self, n, shape, dy, w, pre, accumulate, dx):
    with self.lock:
      check(self._lib.ffn_gradients_conv_backward_input(
          self._h, int(n), _lib.i3(shape), _addr(dy), _addr(w), _addr(pre),
          int(bool(accumulate)), _addr(dx)))

  def conv_backward_weights(self, n, shape, cin, x, x2, relu_in, dy, dw, db):
    with self.lock:
      check(self._lib.ffn_gradients_conv_backward_weights(
          self._h, int(n), _lib.i3(shape), int(cin), _addr(x), _addr(x2),
          int(bool(relu_in)), _addr(dy), _addr(dw), _addr(db)))

  def head_forward(self, n, shape, net, seed, w, b, logits):
    with self.lock:
      check(self._lib.ffn_gradients_head_forward(
          self._h, int(n), _lib.i3(shape), _addr(net), _addr(seed), _addr(w),
          _addr(b), _addr(logits)))

  def head_backward(self, n, shape, net, dlogits, w, dnet, dw, db):
    with self.lock:
      check(self._lib.ffn_gradients_head_backward(
          self._h, int(n), _lib.i3(shape), _addr(net), _addr(dlogits), _addr(w),
          _addr(dnet), _addr(dw), _addr(db)))

  def loss(self, n, shape, logits, labels, weights, dlogits) -> float:
    out = ctypes.c_float(0.0)
    with self.lock:
      check(self._lib.ffn_gradients_loss(
          self._h, int(n), _lib.i3(shape), _addr(logits), _addr(labels),
          _addr(weights), ctypes.byref(out), _addr(dlogits)))
    return float(out.value)

  def last_timing(self):
    """{call name: HIP-event kernel ms of its last run on this handle}."""
    ms = (ctypes.c_double * len(TIMED_CALLS))()
    with self.lock:
      check(self._lib.ffn_gradients_last_timing(self._h, ms))
    return dict(zip(TIMED_CALLS, [float(v) for v in ms]))


_default = _unit.Registry(GradientOps)


def default_ops(device_id: int = 0) -> GradientOps:
  """Process-wide GradientOps of a device (created on first use)."""
  return _default.get(device_id)


class ConvStackGradients:
  """Loss and gradients of a ConvStack3DFFNModel (any depth >= 2, 32 features,
  any FoV) for up to `max_batch` FoVs per call; the weights and every buffer
  live on device `device_id`.

  `storage`, if given, is {'w', 'b', 'dw', 'db'}: per kind a dict scope -> flat
  f32 device tensor of the variable's size, 16-byte aligned.  The object then
  reads its weights from and writes its gradients to these tensors (views into
  a trainer's arenas) instead of allocating its own, and the caller keeps them
  current; the weights are not uploaded from the model."""

  def __init__(self, model, max_batch: int = 1, device_id: int = 0,
               storage=None):
    if model.variables is None:
      raise ValueError('model has no weights (load_checkpoint / init_random)')
    if model.features != FEATURES:
      raise ValueError('features = %d, the kernels are built for %d' %
                       (model.features, FEATURES))
    if model.depth < 2:
      raise ValueError('depth = %d, expected >= 2' % model.depth)
    if not 1 <= int(max_batch) <= MAX_BATCH:
      raise ValueError('max_batch = %r, expected 1 .. %d' %
                       (max_batch, MAX_BATCH))
    # (before the library is loaded: torch brings its own copy of the HIP
    # runtime, and the process must end up with one)
    import torch  # pylint:disable=g-import-not-at-top
    self.ops = GradientOps(device_id)  # raises without a GPU
    self.torch = torch
    self.device = torch.device('cuda', device_id)
    self.depth = int(model.depth)
    self.max_batch = int(max_batch)
    self.scopes = convstack_3d.conv_scopes(self.depth)
    self.shapes = {}
    self.w = {}
    self.b = {}
    self._dw = self._db = None
    if storage is None:
      self.set_variables(model.variables)
    else:
      self._adopt(model.variables, storage)
    self._buffers = None
    self._key = None

  def set_variables(self, variables):
    """Copies the model's variables to the device (again, after an update)."""
    torch = self.torch
    for scope in self.scopes:
      for kind, store in (('weights', self.w), ('biases', self.b)):
        name = 'seed_update/%s/%s' % (scope, kind)
        host = np.ascontiguousarray(variables[name], dtype=np.float32)
        self.shapes[name] = host.shape
        flat = torch.from_numpy(host.reshape(-1).copy())
        if self._dw is None:
          store[scope] = flat.to(self.device)
        else:  # handed storage: in place, the views stay what they are
          store[scope].copy_(flat)
    torch.cuda.synchronize(self.device)

  def _adopt(self, variables, storage):
    torch = self.torch
    for scope in self.scopes:
      for kind, key in (('weights', 'w'), ('biases', 'b')):
        name = 'seed_update/%s/%s' % (scope, kind)
        self.shapes[name] = tuple(np.shape(variables[name]))
        size = int(np.prod(self.shapes[name]))
        for k in (key, 'd' + key):
          t = storage[k][scope]
          if (t.dtype != torch.float32 or t.device != self.device or
              tuple(t.shape) != (size,) or not t.is_contiguous() or
              t.data_ptr() % 16):
            raise ValueError('storage[%r][%r]: expected %d dense f32 on %s, '
                             '16-byte aligned' % (k, scope, size, self.device))
    self.w, self.b = dict(storage['w']), dict(storage['b'])
    self._dw, self._db = dict(storage['dw']), dict(storage['db'])

  def close(self):
    self.ops.close()

  # -- buffers ---------------------------------------------------------------
  def _to_device(self, a, shape):
    torch = self.torch
    if not isinstance(a, torch.Tensor):
      a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    if tuple(a.shape) != tuple(shape):
      raise ValueError('array of shape %r, expected %r' %
                       (tuple(a.shape), tuple(shape)))
    return a.to(self.device, torch.float32).contiguous()

  def _ensure(self, n, zyx):
    key = (n,) + tuple(zyx)
    if self._key == key:
      return self._buffers
    torch = self.torch
    self._buffers = None  # free before allocating the next set
    act = (n,) + tuple(zyx) + (FEATURES,)
    new = lambda shape: torch.empty(shape, dtype=torch.float32,
                                    device=self.device)
    buf = {
        'pre': [new(act) for _ in range(2 * self.depth)],
        'g': new(act), 't': new(act),
        'logits': new(key), 'dlogits': new(key),
        'dw': self._dw or {s: new(self.w[s].shape) for s in self.scopes},
        'db': self._db or {s: new(self.b[s].shape) for s in self.scopes},
    }
    self._buffers, self._key = buf, key
    return buf

  # -- the stack -------------------------------------------------------------
  def loss_and_gradients(self, seed, image, labels, weights,
                         return_pre_activations: bool = False):
    """seed, image, labels, weights: [n, z, y, x], numpy or device arrays.

    Returns (loss, logits, grads) -- or (loss, logits, grads, pre_activations)
    on request: loss a float, logits the updated seed [n, z, y, x], grads a
    dict keyed by the checkpoint's variable names with arrays in the
    checkpoint's shapes, pre_activations the inputs of every ReLU in network
    order (conv0_a's output, then per residual block its incoming stream and
    conv_i_a's output, then the final stream: 2 * depth arrays
    [n, z, y, x, 32]).  All returned arrays are numpy."""
    loss, buf = self._run(seed, image, labels, weights)
    dw, db = buf['dw'], buf['db']
    grads = {}
    for scope in self.scopes:
      for kind, store in (('weights', dw), ('biases', db)):
        name = 'seed_update/%s/%s' % (scope, kind)
        grads[name] = store[scope].cpu().numpy().reshape(self.shapes[name])
    logits = buf['logits'].cpu().numpy()
    if return_pre_activations:
      return loss, logits, grads, [p.cpu().numpy() for p in buf['pre']]
    return loss, logits, grads

  def loss_and_gradients_device(self, seed, image, labels, weights):
    """The same calls; returns (loss, logits) with logits a device tensor
    [n, z, y, x] that the next call overwrites.  The gradients stay on the
    device: in the handed storage, or in this object's own buffers."""
    loss, buf = self._run(seed, image, labels, weights)
    return loss, buf['logits']

  def _run(self, seed, image, labels, weights):
    """Forward and backward through the unit; returns (loss, buffers)."""
    shape4 = tuple(int(v) for v in np.shape(seed))
    if len(shape4) != 4:
      raise ValueError('expected [n, z, y, x] arrays, got shape %r' % (shape4,))
    n, zyx = shape4[0], shape4[1:]
    if not 1 <= n <= self.max_batch:
      raise ValueError('batch of %d, this object takes 1 .. %d' %
                       (n, self.max_batch))
    torch, ops, depth = self.torch, self.ops, self.depth
    seed_d = self._to_device(seed, shape4)
    image_d = self._to_device(image, shape4)
    labels_d = self._to_device(labels, shape4)
    weights_d = self._to_device(weights, shape4)
    buf = self._ensure(n, zyx)
    pre, g, t = buf['pre'], buf['g'], buf['t']
    w, b, dw, db = self.w, self.b, buf['dw'], buf['db']
    torch.cuda.synchronize(self.device)  # the unit runs on its own stream

    # forward (convstack_3d.py:38-54); pre[k] is what the k-th ReLU reads
    ops.conv_forward(n, zyx, 2, image_d, seed_d, False, w['conv0_a'],
                     b['conv0_a'], None, pre[0])
    ops.conv_forward(n, zyx, FEATURES, pre[0], None, True, w['conv0_b'],
                     b['conv0_b'], None, pre[1])
    for i in range(1, depth):
      a, c = 'conv%d_a' % i, 'conv%d_b' % i
      stream, mid, out = pre[2 * i - 1], pre[2 * i], pre[2 * i + 1]
      ops.conv_forward(n, zyx, FEATURES, stream, None, True, w[a], b[a], None,
                       mid)
      ops.conv_forward(n, zyx, FEATURES, mid, None, True, w[c], b[c], stream,
                       out)
    final = pre[2 * depth - 1]
    ops.head_forward(n, zyx, final, seed_d, w['conv_lom'], b['conv_lom'],
                     buf['logits'])
    loss = ops.loss(n, zyx, buf['logits'], labels_d, weights_d, buf['dlogits'])

    # backward; g holds d loss / d stream
    ops.head_backward(n, zyx, final, buf['dlogits'], w['conv_lom'], g,
                      dw['conv_lom'], db['conv_lom'])
    for i in range(depth - 1, 0, -1):
      a, c = 'conv%d_a' % i, 'conv%d_b' % i
      stream, mid = pre[2 * i - 1], pre[2 * i]
      ops.conv_backward_weights(n, zyx, FEATURES, mid, None, True, g, dw[c],
                                db[c])
      ops.conv_backward_input(n, zyx, g, w[c], mid, False, t)
      ops.conv_backward_weights(n, zyx, FEATURES, stream, None, True, t, dw[a],
                                db[a])
      ops.conv_backward_input(n, zyx, t, w[a], stream, True, g)
    ops.conv_backward_weights(n, zyx, FEATURES, pre[0], None, True, g,
                              dw['conv0_b'], db['conv0_b'])
    ops.conv_backward_input(n, zyx, g, w['conv0_b'], pre[0], False, t)
    ops.conv_backward_weights(n, zyx, 2, image_d, seed_d, False, t,
                              dw['conv0_a'], db['conv0_a'])
    return loss, buf
