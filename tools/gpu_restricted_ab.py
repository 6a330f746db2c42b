#!/usr/bin/env python3
"""What a restricted canvas costs: complete `segment_all` passes (PolicyPeaks)
over bench.py's 250^3 volume under a MovementRestrictor with all three parts,
the arms taking turns in one process:
  native      the library's loop and turn (the restrictor on the device,
              ffn_canvas_set_restrictor);
  python_turn the Python loop (a NATIVE_LOOP = False subclass), the device turn;
  python      the Python loop and one device call per question between two
              segments: the path every restricted canvas took before the
              restrictor could be uploaded.
The arms must agree on the segmentation and on the counters that count work.

  python tools/gpu_restricted_ab.py [--passes 2] [--out profiles/...txt]
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from ffn_amd import synthetic  # noqa: E402
from ffn_amd.inference import executor  # noqa: E402
from ffn_amd.inference import inference  # noqa: E402
from ffn_amd.inference import inference_utils  # noqa: E402
from ffn_amd.inference import movement  # noqa: E402
from ffn_amd.inference import seed as seed_lib  # noqa: E402

WORK = ('update_at-calls', 'skip_restriced_pos', 'skip_threshold',
        'skip_invalid_pos', 'seed_got_too_weak', 'voxels-segmented')


class _Box:

  def __init__(self, start, size):
    self.start = np.array(start)
    self.end = self.start + np.array(size)


class PythonLoopCanvas(inference.DeviceCanvas):
  NATIVE_LOOP = False


class NoUploadCanvas(PythonLoopCanvas):
  """The restrictor stays on the host: Python loop, no device turn."""

  def _upload_restrictor(self):
    self.__dict__.pop('_native_ok', None)
    self.__dict__.pop('_turn_static', None)
    self._restrict_on = False
    self.restrictor_upload_seconds = 0.0


ARMS = {'native': inference.DeviceCanvas, 'python_turn': PythonLoopCanvas,
        'python': NoUploadCanvas}


def restrictor(shape):
  """mask: a slab across z plus a vertical cylinder; seed mask: a box; an f32
  shift field at scale 2 with two patches >= 4, FoV start (-6, -6, -4) xyz,
  size (13, 13, 9)."""
  z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
  mask = np.broadcast_to((z >= 120) & (z < 128), shape) | np.broadcast_to(
      (y - 80) ** 2 + (x - 170) ** 2 <= 20 ** 2, shape)
  seed_mask = np.zeros(shape, bool)
  seed_mask[20:80, 20:110, 30:120] = True
  shift = np.zeros((2, shape[0], shape[1] // 2, shape[2] // 2), np.float32)
  shift[0, 180:196, 20:28, 60:68] = 5.0
  shift[1, 40:52, 90:96, 10:18] = -4.5
  return movement.MovementRestrictor(
      mask=np.ascontiguousarray(mask), seed_mask=seed_mask, shift_mask=shift,
      shift_mask_fov=_Box((-6, -6, -4), (13, 13, 9)), shift_mask_threshold=4,
      shift_mask_scale=2)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--passes', type=int, default=2, help='per arm')
  ap.add_argument('--volume', type=int, default=250)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  model = bench.load_model()
  request = bench.make_request()
  shape = (args.volume,) * 3
  image = synthetic.normalize(bench.bench_volume(shape, seed=1234))
  r = restrictor(shape)
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), model, model.info,
                                  None, inference_utils.Counters(), 1, device_id=0)
  rows, results = [], {}
  try:
    for k in range(len(ARMS) * args.passes):
      arm = list(ARMS)[k % len(ARMS)]
      cls = ARMS[arm]
      counters = inference_utils.Counters()
      canvas = cls(model.info, exe.get_client(counters, direct=True), image,
                   request.inference_options, counters=counters, restrictor=r,
                   movement_policy_fn=movement.get_policy_fn(request, model.info))
      assert canvas._native_loop_ok() == (arm == 'native')
      assert canvas._turn_ok() == (arm != 'python')
      exe.engine.synchronize()
      t0 = time.perf_counter()
      canvas.segment_all(seed_policy=seed_lib.PolicyPeaks)
      exe.engine.synchronize()
      dt = time.perf_counter() - t0
      steps = counters['update_at-calls'].value
      row = dict(arm=arm, seconds=round(dt, 3), steps=steps,
                 fov_steps_per_s=round(steps / dt, 1), turns=canvas.turns,
                 segments=len(canvas.origins),
                 set_restrictor_ms=round(1e3 * canvas.restrictor_upload_seconds, 2),
                 work={key: counters[key].value for key in WORK})
      rows.append(row)
      print(json.dumps(row), flush=True)
      results.setdefault(arm, []).append(
          (np.array(np.asarray(canvas.segmentation)), row['work']))
      canvas.close()
  finally:
    exe.engine.close()
  ref_seg, ref_work = results['native'][0]
  agree = all(np.array_equal(seg, ref_seg) and work == ref_work
              for arm in results for seg, work in results[arm])
  rate = {arm: float(np.median([x['fov_steps_per_s'] for x in rows if x['arm'] == arm]))
          for arm in results}
  summary = dict(box=platform.node(), volume=list(shape), passes_per_arm=args.passes,
                 arms_agree=agree, median_fov_steps_per_s=rate,
                 native_over_python=round(rate['native'] / rate['python'], 3),
                 native_over_python_turn=round(rate['native'] / rate['python_turn'], 3))
  print(json.dumps(summary), flush=True)
  if args.out:
    with open(args.out, 'w') as f:
      f.write('# tools/gpu_restricted_ab.py --passes %d (%s)\n' % (
          args.passes, time.strftime('%Y-%m-%d %H:%M:%S')))
      for row in rows:
        f.write(json.dumps(row) + '\n')
      f.write(json.dumps(summary) + '\n')
  if not agree:
    sys.exit('the arms disagree')


if __name__ == '__main__':
  main()
