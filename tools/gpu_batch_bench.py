#!/usr/bin/env python3
"""Config C3 shape: B concurrent canvases on one MI355X, FoV steps batched by the
executor's server thread into single ffn_canvas_step(n, ...) calls.

  python tools/gpu_batch_bench.py --canvases 8 --batch 8 --size 160 --steps 400

--mode products: same-process A/B of engine option mfma_products (3: the f32-accurate
split product, 1: fp16 inference), the arms taking turns leg by leg --
  * the conv stack alone on FoVs resident in the engine (conv32m) at --batches: us per
    FoV-conv from the event pair around each stack's convs, with board power and sclk
    sampled while the leg runs (bench.BoardSampler);
  * --canvases canvases under MultiCanvasDriver (--batch per call): FoV-steps/s.

  python tools/gpu_batch_bench.py --mode products --batches 8,16 --canvases 16 --batch 16
"""
import argparse
import functools
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from ffn_amd import synthetic  # noqa: E402
from ffn_amd.inference import executor, inference, inference_utils  # noqa: E402
from ffn_amd.inference import movement, seed as seed_lib  # noqa: E402


class _Done(Exception):
  pass


def run_driver(args, model, request, counters):
  """Same workload through the single-threaded MultiCanvasDriver."""
  for overlap in (False, True):
    exe = executor.HipBatchExecutor(executor.ExecutorInterface(), model,
                                    model.info, None, counters, args.batch)
    jobs = []
    for k in range(args.canvases):
      vol = synthetic.normalize(synthetic.cells_volume((args.size,) * 3,
                                                       seed=100 + k))
      sub = counters.get_sub_counters()
      canvas = inference.DeviceCanvas(
          model.info, exe.get_client(sub, direct=True), vol,
          request.inference_options, counters=sub,
          movement_policy_fn=movement.get_policy_fn(request, model.info))
      jobs.append((canvas, functools.partial(seed_lib.PolicyGrid3d, step=16,
                                             offsets=(0, 8, 4, 12))))
    drv = inference.MultiCanvasDriver(exe.engine, args.batch, overlap=overlap,
                                      max_steps_per_canvas=args.steps)
    t0 = time.perf_counter()
    drv.run(jobs)
    exe.engine.synchronize()
    dt = time.perf_counter() - t0
    print('driver overlap=%d canvases %d batch %d: %d steps in %.2f s = %.1f '
          'FoV-steps/s; %d engine calls (mean fill %.2f)' %
          (overlap, args.canvases, args.batch, drv.steps, dt, drv.steps / dt,
           drv.calls, drv.steps / max(drv.calls, 1)))
    for canvas, _ in jobs:
      canvas.close()
    exe.engine.close()


def _driver_leg(args, model, request, counters, products):
  """FoV-steps/s of one MultiCanvasDriver run on a fresh engine with `products`."""
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), model, model.info, None,
                                  counters, args.batch)
  exe.engine.set_option('mfma_products', products)
  jobs = []
  for k in range(args.canvases):
    vol = synthetic.normalize(synthetic.cells_volume((args.size,) * 3, seed=100 + k))
    sub = counters.get_sub_counters()
    canvas = inference.DeviceCanvas(
        model.info, exe.get_client(sub, direct=True), vol, request.inference_options,
        counters=sub, movement_policy_fn=movement.get_policy_fn(request, model.info))
    jobs.append((canvas, functools.partial(seed_lib.PolicyGrid3d, step=16,
                                           offsets=(0, 8, 4, 12))))
  drv = inference.MultiCanvasDriver(exe.engine, args.batch,
                                    max_steps_per_canvas=args.steps)
  t0 = time.perf_counter()
  drv.run(jobs)
  exe.engine.synchronize()
  dt = time.perf_counter() - t0
  variant = exe.engine.get_option('conv_variant')
  for canvas, _ in jobs:
    canvas.close()
  exe.engine.close()
  return drv.steps / dt, drv.steps, drv.steps / max(drv.calls, 1), variant


def run_products(args, model, request, counters):
  """A/B of mfma_products = 3 / 1: the batched conv stack, then the batched loop."""
  import numpy as np
  from ffn_amd import engine as hip_engine
  batches = [int(b) for b in args.batches.split(',') if b]
  n_convs = 2 * model.depth - 1
  eng = hip_engine.HipEngine.from_model(model, max_batch=max(batches))
  eng.set_option('conv_variant', 8)  # conv32m for every batch, as the batched drivers pin it
  eng.set_option('profile_every', 1)
  rng = np.random.RandomState(0)
  fov = eng.fov_zyx
  img = rng.normal(0, 1, (max(batches),) + fov).astype(np.float32)
  seed = np.full(img.shape, -2.944, np.float32)
  for n in batches:
    eng.predict(seed[:n], img[:n])  # the FoVs of the legs, resident from here on
    us = {3: [], 1: []}
    board = {3: [], 1: []}
    for leg in range(args.warm_legs + args.legs):
      for products in (3, 1):
        eng.set_option('mfma_products', products)
        eng.set_profiling(2)
        eng.get_profile(reset=True)
        with bench.BoardSampler(0, period_s=0.002) as bs:
          eng.forward_resident(n, args.leg_stacks)
          eng.synchronize()
        ms = eng.get_profile_samples()
        eng.set_profiling(0)
        if leg < args.warm_legs or not len(ms):
          continue
        us[products].append(float(np.median(ms)) * 1e3 / (n_convs * n))
        if bs.power_w:
          half = len(bs.power_w) // 2
          board[products].append((float(np.median(bs.power_w[half:])),
                                  float(np.median(bs.sclk_mhz[half:]))))
    for products in (3, 1):
      t = np.array(us[products])
      line = ('conv32m batch %d, mfma_products %d: median %.3f us per FoV-conv (min %.3f, '
              'max %.3f) over %d legs of %d stacks' % (
                  n, products, np.median(t), t.min(), t.max(), len(t), args.leg_stacks))
      if board[products]:
        b = np.array(board[products])
        line += '; board %.0f W, sclk %.0f MHz' % (np.median(b[:, 0]), np.median(b[:, 1]))
      print(line, flush=True)
    print('conv32m batch %d: one product takes %.3f of three' % (
        n, np.median(us[1]) / np.median(us[3])), flush=True)
  eng.close()
  if args.canvases:
    rates = {3: [], 1: []}
    for _ in range(args.driver_rounds):
      for products in (3, 1):
        rate, steps, fill, variant = _driver_leg(args, model, request, counters, products)
        rates[products].append(rate)
        print('driver canvases %d batch %d, mfma_products %d (conv_variant %d): %d steps, '
              '%.1f FoV-steps/s, mean fill %.2f' % (
                  args.canvases, args.batch, products, variant, steps, rate, fill),
              flush=True)
    print('driver: one product runs at %.3f of three products\' FoV-steps/s (medians)' % (
        np.median(rates[1]) / np.median(rates[3])), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--canvases', type=int, default=8)
  ap.add_argument('--batch', type=int, default=8)
  ap.add_argument('--size', type=int, default=160)
  ap.add_argument('--steps', type=int, default=400, help='per canvas')
  ap.add_argument('--mode', choices=['threads', 'driver', 'products'], default='threads')
  ap.add_argument('--batches', default='8,16', help='products: batches of the conv legs')
  ap.add_argument('--legs', type=int, default=6, help='products: per arm')
  ap.add_argument('--warm-legs', type=int, default=1)
  ap.add_argument('--leg-stacks', type=int, default=40, help='products: stacks per leg')
  ap.add_argument('--driver-rounds', type=int, default=2)
  args = ap.parse_args()
  model = bench.load_model()
  request = bench.make_request()
  counters = inference_utils.Counters()
  if args.mode == 'driver':
    return run_driver(args, model, request, counters)
  if args.mode == 'products':
    return run_products(args, model, request, counters)
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), model,
                                  model.info, None, counters, args.batch,
                                  expected_clients=args.canvases)
  exe.start_server()
  vols = [synthetic.normalize(synthetic.cells_volume((args.size,) * 3,
                                                     seed=100 + k))
          for k in range(args.canvases)]
  start = threading.Barrier(args.canvases + 1)
  done_steps = [0] * args.canvases

  def work(k):
    sub = counters.get_sub_counters()

    class C(inference.DeviceCanvas):

      def update_at(self, pos):
        r = super().update_at(pos)
        done_steps[k] += 1
        if done_steps[k] >= args.steps:
          raise _Done()
        return r

    canvas = C(model.info, exe.get_client(sub), vols[k],
               request.inference_options, counters=sub,
               movement_policy_fn=movement.get_policy_fn(request, model.info))
    start.wait()
    try:
      canvas.segment_all(seed_policy=functools.partial(
          seed_lib.PolicyGrid3d, step=16, offsets=(0, 8, 4, 12)))
    except _Done:
      pass
    canvas._deregister_client()

  threads = [threading.Thread(target=work, args=(k,), daemon=True)
             for k in range(args.canvases)]
  for t in threads:
    t.start()
  start.wait()
  t0 = time.perf_counter()
  for t in threads:
    t.join()
  dt = time.perf_counter() - t0
  exe.stop_server()
  total = sum(done_steps)
  calls = counters['executor-inference-calls'].value
  print('canvases %d batch %d: %d steps in %.2f s = %.1f FoV-steps/s; '
        '%d engine calls (mean fill %.2f)' %
        (args.canvases, args.batch, total, dt, total / dt, calls,
         total / max(calls, 1)))


if __name__ == '__main__':
  main()
