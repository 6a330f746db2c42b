// Canvas utility kernels: box reads / writes / fills, commit, the between-segment turn (integer / byte work, HBM-bound).
// (included by ffn_canvas.hip alone, behind ffn_kernels.h, inside no namespace)
#pragma once

namespace ffn {

// ---------------------------------------------------------------------------
// Canvas utility kernels (integer / byte work, HBM-bound).
// ---------------------------------------------------------------------------
struct Box {
  int lo[3];
  int n[3];      // extent
  int cy, cx;    // canvas strides
};

__device__ __forceinline__ size_t box_index(const Box& b, long e) {
  const int x = e % b.n[2];
  const long t = e / b.n[2];
  const int y = t % b.n[1];
  const int z = t / b.n[1];
  return ((size_t)(b.lo[0] + z) * b.cy + (b.lo[1] + y)) * b.cx + (b.lo[2] + x);
}

template <typename T>
__global__ void box_read_kernel(const T* __restrict__ vol, Box b, long total,
                                T* __restrict__ dst) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total;
       e += (long)gridDim.x * blockDim.x)
    dst[e] = vol[box_index(b, e)];
}

template <typename T>
__global__ void box_write_kernel(T* __restrict__ vol, Box b, long total,
                                 const T* __restrict__ src) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total;
       e += (long)gridDim.x * blockDim.x)
    vol[box_index(b, e)] = src[e];
}

template <typename T>
__global__ void box_fill_kernel(T* __restrict__ vol, Box b, long total, T value) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total;
       e += (long)gridDim.x * blockDim.x)
    vol[box_index(b, e)] = value;
}

__global__ void fill_u32_kernel(uint32_t* __restrict__ p, uint32_t v, size_t n) {
  // 16-byte stores, grid-stride: the per-seed "seed.clear()" (storage.py:69-71).
  const size_t n4 = n / 4;
  uint4 vv = make_uint4(v, v, v, v);
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n4;
       e += (size_t)gridDim.x * blockDim.x)
    reinterpret_cast<uint4*>(p)[e] = vv;
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) p[n4 * 4 + threadIdx.x] = v;
}

__global__ void points_read_kernel(const float* __restrict__ seed,
                                   const int32_t* __restrict__ seg, int cz,
                                   int cy, int cx, int n,
                                   const int32_t* __restrict__ pos,
                                   float* __restrict__ seed_out,
                                   int32_t* __restrict__ seg_out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int z = pos[3 * k], y = pos[3 * k + 1], x = pos[3 * k + 2];
  if (z < 0 || z >= cz || y < 0 || y >= cy || x < 0 || x >= cx) {
    seed_out[k] = __builtin_nanf("");
    seg_out[k] = 0;
    return;
  }
  const size_t ci = ((size_t)z * cy + y) * cx + x;
  seed_out[k] = seed[ci];
  seg_out[k] = seg[ci];
}

__global__ void points_write_seg_kernel(int32_t* __restrict__ seg, int cy, int cx,
                                        int n, const int32_t* __restrict__ pos,
                                        const int32_t* __restrict__ val) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  seg[((size_t)pos[3 * k] * cy + pos[3 * k + 1]) * cx + pos[3 * k + 2]] = val[k];
}

__global__ void set_seg_point_kernel(int32_t* __restrict__ seg, size_t ci,
                                     int32_t value) {
  seg[ci] = value;
}

__global__ void set_seed_point_kernel(float* __restrict__ seed, size_t ci,
                                      float value) {
  seed[ci] = value;
}

__global__ void any_segmented_kernel(const int32_t* __restrict__ seg, Box b,
                                     long total, int32_t* __restrict__ out) {
  int hit = 0;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total;
       e += (long)gridDim.x * blockDim.x)
    hit |= seg[box_index(b, e)] > 0;
  if (__any(hit) && (threadIdx.x & 63) == 0) atomicOr(out, 1);
}

// ---------------------------------------------------------------------------
// Box sweeps of the commit and of the between-segment turn: rows of the box dealt
// to the waves of the grid.  z and y come from one division per row, x runs
// contiguously along the lanes (no 64-bit / or % per voxel, box_index above).  A
// box narrower than a wave puts 64 >> xs rows side by side (xs: log2 of the lanes
// a row gets, row_lanes_log2 on the host).  f(ci) is called once per voxel.
// ---------------------------------------------------------------------------
// (kTurnBlocks, the grid cap of these sweeps = partial sums per count: ffn_types.h)
constexpr int kTurnHistLds = 4096;  // max_existing_id + 1 <= this: overlaps counted in LDS

template <typename F>
__device__ __forceinline__ void for_box_rows(const Box& b, long rows, int xs, F&& f) {
  const int lane = threadIdx.x & 63;
  const int per = 64 >> xs;
  const int sub = lane >> xs, x0 = lane & ((1 << xs) - 1);
  const long wave = blockIdx.x * (long)(blockDim.x >> 6) + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * (blockDim.x >> 6);
  for (long r = wave * per + sub; r < rows; r += nwaves * per) {
    const long z = r / b.n[1];
    const int y = (int)(r - z * b.n[1]);
    const size_t base =
        ((size_t)(b.lo[0] + z) * b.cy + (b.lo[1] + y)) * b.cx + b.lo[2];
    for (int x = x0; x < b.n[2]; x += 1 << xs) f(base + x);
  }
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, off);
    const unsigned hi = __shfl_xor((unsigned)(v >> 32), off);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// partials[2 * block] = raw, [2 * block + 1] = actual of the block's rows (every
// block writes its pair: nothing to zero, no atomics on the totals); hist[id] += 1
// for overlapped ids in [1, max_id].  lds_hist (max_id < kTurnHistLds): the block
// counts in LDS and adds each non-zero bin to `hist` once; otherwise one global
// atomic per overlapped voxel.  `hist` is all zero when the kernel starts
// (turn_publish_kernel leaves it so).
__global__ __launch_bounds__(256) void turn_count_kernel(
    const float* __restrict__ seed, const int32_t* __restrict__ seg, Box b, long rows,
    int xs, float thr, int32_t max_id, int lds_hist,
    unsigned long long* __restrict__ partials, unsigned* __restrict__ hist) {
  __shared__ unsigned s_hist[kTurnHistLds];
  __shared__ unsigned s_red[2][4];
  const int bins = lds_hist ? max_id + 1 : 0;
  for (int i = threadIdx.x; i < bins; i += 256) s_hist[i] = 0;
  __syncthreads();
  unsigned raw = 0, act = 0;
  for_box_rows(b, rows, xs, [&](size_t ci) {
    const float v = seed[ci];
    const int32_t s = seg[ci];
    if (v >= thr) {  // NaN -> false
      ++raw;
      if (s <= 0) {
        ++act;
      } else if (s <= max_id) {
        if (lds_hist)
          atomicAdd(&s_hist[s], 1u);
        else
          atomicAdd(&hist[s], 1u);
      }
    }
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    raw += __shfl_xor(raw, off);
    act += __shfl_xor(act, off);
  }
  if ((threadIdx.x & 63) == 0) {
    s_red[0][threadIdx.x >> 6] = raw;
    s_red[1][threadIdx.x >> 6] = act;
  }
  __syncthreads();
  for (int i = 1 + threadIdx.x; i < bins; i += 256) {
    const unsigned n = s_hist[i];
    if (n) atomicAdd(&hist[i], n);
  }
  if (threadIdx.x == 0) {
    unsigned long long r = 0, a = 0;
    for (int w = 0; w < 4; ++w) {
      r += s_red[0][w];
      a += s_red[1][w];
    }
    partials[2 * blockIdx.x] = r;
    partials[2 * blockIdx.x + 1] = a;
  }
}

__global__ void commit_assign_kernel(const float* __restrict__ seed,
                                     int32_t* __restrict__ seg, Box b, long total,
                                     float thr, int32_t sid) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total;
       e += (long)gridDim.x * blockDim.x) {
    const size_t ci = box_index(b, e);
    if (seed[ci] >= thr && seg[ci] <= 0) seg[ci] = sid;
  }
}

// ---------------------------------------------------------------------------
// The between-segment turn of Canvas.segment_all (inference.py:573-660) as ONE
// device-side sequence (ffn_canvas_segment_turn): commit count -> assign if the
// object is large enough (else the -1 marker at its seed) -> the next seeds of
// the policy tested in order (already segmented / too close to a segment, the
// latter marked -1) -> the canvas' seed volume re-initialised at the first one
// that passes -> everything the host reads published into pinned memory, which
// the host polls: at most five launches (count, commit, evaluate, pick + clear,
// publish), no memset, no copy operation, no stream wait.  Phases that depend on
// each other are separate launches: no workgroup waits for another.
// ---------------------------------------------------------------------------
// (the record of a turn, TurnRecord: ffn_types.h)
constexpr int kTurnOk = 0, kTurnSegmented = 1, kTurnTooClose = 2, kTurnNotReached = 3,
              kTurnRestricted = 4;

// Every block sums the count's partials for itself (64-bit) and decides; block 0
// writes the record.  nparts = 0: no commit asked for, or an empty box.
// mark_mode 0: no marker; 1: seg[mark] = -1 if it is 0 (inference.py:600-603, a
// seed that got too weak); 2: the same, but only when nothing is committed
// (inference.py:632-636, too small).  A marker voxel that this launch's own
// assign loop gives the id to is left to that loop: the commit comes first.
__global__ __launch_bounds__(256) void turn_commit_kernel(
    const float* __restrict__ seed, int32_t* __restrict__ seg, Box b, long rows, int xs,
    float thr, int32_t sid, long long min_size,
    const unsigned long long* __restrict__ partials, int nparts,
    TurnRecord* __restrict__ rec, int mz, int my, int mx, int mark_mode) {
  __shared__ unsigned long long s_red[2][4];
  unsigned long long raw = 0, act = 0;
  for (int i = threadIdx.x; i < nparts; i += 256) {
    raw += partials[2 * i];
    act += partials[2 * i + 1];
  }
  raw = wave_sum_u64(raw);
  act = wave_sum_u64(act);
  if ((threadIdx.x & 63) == 0) {
    s_red[0][threadIdx.x >> 6] = raw;
    s_red[1][threadIdx.x >> 6] = act;
  }
  __syncthreads();
  raw = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
  act = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
  const bool ok = nparts > 0 && (long long)act >= min_size;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    rec->counts[0] = raw;
    rec->counts[1] = act;
    rec->committed = ok ? 1 : 0;
    rec->chosen = -1;
    if (mark_mode == 1 || (mark_mode == 2 && !ok)) {
      const size_t mci = ((size_t)mz * b.cy + my) * b.cx + mx;
      const bool in_box = mz >= b.lo[0] && mz < b.lo[0] + b.n[0] && my >= b.lo[1] &&
                          my < b.lo[1] + b.n[1] && mx >= b.lo[2] && mx < b.lo[2] + b.n[2];
      const bool assigned = ok && in_box && seed[mci] >= thr;
      if (!assigned && seg[mci] == 0) seg[mci] = -1;
    }
  }
  if (ok)
    for_box_rows(b, rows, xs, [&](size_t ci) {
      if (seed[ci] >= thr && seg[ci] <= 0) seg[ci] = sid;
    });
}

// one wavefront per candidate: segmentation[pos] > 0 (Canvas.is_valid_pos,
// inference.py:341), else a restrictor veto (MovementRestrictor.is_valid_pos /
// is_valid_seed, inference.py:573-574: the reference moves on before the
// too-close test, so no marker), else any id > 0 in the clipped box
// pos +- min_boundary_dist (inference.py:575-581).  rplanes: the canvas'
// restriction bit planes (ffn_restrict_kernels.h), NULL without a restrictor.
// cand: the host's pinned, device-mapped list (no copy operation; read here only:
// the later kernels take the voxel index from cand_ci).
__global__ __launch_bounds__(64) void turn_eval_kernel(
    const float* __restrict__ seed, const int32_t* __restrict__ seg, int cz, int cy,
    int cx, const int32_t* __restrict__ cand, int mz, int my, int mx,
    int* __restrict__ flags, float* __restrict__ cand_seed,
    int32_t* __restrict__ cand_seg, size_t* __restrict__ cand_ci,
    const unsigned long long* __restrict__ rplanes, size_t plane_words, int row_words) {
  const int j = blockIdx.x;
  const int z = cand[3 * j], y = cand[3 * j + 1], x = cand[3 * j + 2];
  const size_t ci = ((size_t)z * cy + y) * cx + x;
  const int32_t s = seg[ci];
  int flag = kTurnOk;
  bool restricted = false;
  if (rplanes) {
    const size_t wi = ((size_t)z * cy + y) * row_words + (x >> 6);
    restricted = ((rplanes[wi] | rplanes[plane_words + wi]) >> (x & 63)) & 1ull;
  }
  if (s > 0) {
    flag = kTurnSegmented;
  } else if (restricted) {
    flag = kTurnRestricted;
  } else {
    const int z0 = max(z - mz, 0), z1 = min(z + mz + 1, cz);
    const int y0 = max(y - my, 0), y1 = min(y + my + 1, cy);
    const int x0 = max(x - mx, 0), x1 = min(x + mx + 1, cx);
    const int ny = y1 - y0, nx = x1 - x0;
    const int total = (z1 - z0) * ny * nx;
    int hit = 0;
    for (int e = threadIdx.x; e < total; e += 64) {
      const int ex = e % nx, t = e / nx;
      hit |= seg[((size_t)(z0 + t / ny) * cy + (y0 + t % ny)) * cx + (x0 + ex)] > 0;
    }
    if (__any(hit)) flag = kTurnTooClose;
  }
  if (threadIdx.x == 0) {
    flags[j] = flag;
    cand_seed[j] = seed[ci];
    cand_seg[j] = s;
    cand_ci[j] = ci;
  }
}

// Pick, then Canvas.init_seed (inference.py:282-286) at the chosen candidate, in one
// launch.  Every wave finds the first candidate that passed for itself (n flags,
// written by the launch before: nothing to wait for); block 0 gives the too-close
// ones BEFORE it their -1 (the ones after it have not been looked at as far as the
// caller is concerned: turn_publish_kernel reports them as not reached) and writes
// rec->chosen.  clear 0: pick only; 1: the dirty box `b` back to NaN; 2: the whole
// volume, 16-byte stores (the box is at least half of it).  The thread that clears
// the chosen voxel writes the seed value instead; if the voxel lies outside the box
// (or the box is empty, rows = 0) one thread writes it.
__global__ __launch_bounds__(256) void turn_pick_clear_kernel(
    uint32_t* __restrict__ seed, int32_t* __restrict__ seg,
    const int* __restrict__ flags, const size_t* __restrict__ cand_ci, int n,
    TurnRecord* __restrict__ rec, Box b, long rows, int xs, int clear, size_t nvox,
    uint32_t init_bits) {
  const int lane = threadIdx.x & 63;
  int chosen = -1;
  for (int base = 0; base < n && chosen < 0; base += 64) {
    const int j = base + lane;
    const unsigned long long m = __ballot(j < n && flags[j] == kTurnOk);
    if (m) chosen = base + __ffsll((long long)m) - 1;
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    const int upto = chosen < 0 ? n : chosen;
    for (int j = lane; j < upto; j += 64)
      if (flags[j] == kTurnTooClose) seg[cand_ci[j]] = -1;
    if (lane == 0) rec->chosen = chosen;
  }
  if (chosen < 0 || clear == 0) return;
  const size_t cci = cand_ci[chosen];
  constexpr uint32_t kNan = 0x7fc00000u;
  if (clear == 2) {
    const size_t n4 = nvox / 4;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n4;
         e += (size_t)gridDim.x * blockDim.x) {
      uint4 vv = make_uint4(kNan, kNan, kNan, kNan);
      if ((cci >> 2) == e) {
        const int k = (int)(cci & 3);
        if (k == 0) vv.x = init_bits;
        if (k == 1) vv.y = init_bits;
        if (k == 2) vv.z = init_bits;
        if (k == 3) vv.w = init_bits;
      }
      reinterpret_cast<uint4*>(seed)[e] = vv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (nvox & 3)) {
      const size_t ci = n4 * 4 + threadIdx.x;
      seed[ci] = ci == cci ? init_bits : kNan;
    }
    return;
  }
  for_box_rows(b, rows, xs,
               [&](size_t ci) { seed[ci] = ci == cci ? init_bits : kNan; });
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const size_t zy = cci / b.cx;
    const long x = (long)(cci - zy * b.cx), z = (long)(zy / b.cy),
               y = (long)(zy - (size_t)z * b.cy);
    const bool in_box = rows > 0 && z >= b.lo[0] && z < b.lo[0] + b.n[0] &&
                        y >= b.lo[1] && y < b.lo[1] + b.n[1] && x >= b.lo[2] &&
                        x < b.lo[2] + b.n[2];
    if (!in_box) seed[cci] = init_bits;
  }
}

// What the host reads, into pinned host memory as 8-byte words whose upper half is
// the turn's sequence number (faces_body publishes a step's record the same way:
// 8-byte stores are atomic, a word is either an older turn's or this one's; the host
// polls, no stream wait).  One block.
//   pub[0..7]            raw lo, hi; actual lo, hi; committed; chosen; the exact
//                        number of overlapped ids; the number of pairs below
//   pub[8 .. 8 + 3 n)    flags (kTurnNotReached after the chosen one), seed, seg
//   pub[8 + 3 n ...)     the overlaps compacted to (id, count) pairs in ascending id
//                        order, the first max_overlaps of them
// The histogram bins read here go back to zero: the scratch is clean for the next
// turn.  has_commit: turn_commit_kernel wrote the record's counts; otherwise the
// totals are the partials' sums (ffn_canvas_commit_count; nparts = 0: zero).
// has_pick: turn_pick_clear_kernel wrote rec->chosen.
__global__ __launch_bounds__(1024) void turn_publish_kernel(
    const TurnRecord* __restrict__ rec, const unsigned long long* __restrict__ partials,
    int nparts, unsigned* __restrict__ hist, int32_t max_id, int max_overlaps,
    const int* __restrict__ flags, const float* __restrict__ cand_seed,
    const int32_t* __restrict__ cand_seg, int n, int has_commit, int has_pick,
    unsigned long long* __restrict__ pub, unsigned seq) {
  __shared__ unsigned s_w[2][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long tag = (unsigned long long)seq << 32;
  auto put = [&](size_t k, uint32_t v) {
    __hip_atomic_store(&pub[k], tag | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  };
  const int chosen = has_pick ? rec->chosen : -1;
  for (int j = tid; j < n; j += 1024) {
    put(8 + j, (uint32_t)(chosen >= 0 && j > chosen ? kTurnNotReached : flags[j]));
    put(8 + n + j, __float_as_uint(cand_seed[j]));
    put(8 + 2 * (size_t)n + j, (uint32_t)cand_seg[j]);
  }
  const size_t o_pairs = 8 + 3 * (size_t)n;
  unsigned running = 0;
  int it = 0;
  for (long base = 1; base <= max_id; base += 1024, it ^= 1) {
    const long id = base + tid;
    const unsigned cnt = id <= max_id ? hist[id] : 0u;
    if (cnt) hist[id] = 0;
    const unsigned long long m = __ballot(cnt != 0);
    if (lane == 0) s_w[it][wave] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const unsigned v = s_w[it][w];
      all += v;
      if (w < wave) before += v;
    }
    if (cnt) {
      const unsigned idx =
          running + before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
      if (idx < (unsigned)max_overlaps) {
        put(o_pairs + 2 * (size_t)idx, (uint32_t)id);
        put(o_pairs + 2 * (size_t)idx + 1, cnt);
      }
    }
    running += all;
  }
  if (wave == 0) {
    unsigned long long raw = 0, act = 0;
    int committed = 0;
    if (has_commit) {
      raw = rec->counts[0];
      act = rec->counts[1];
      committed = rec->committed;
    } else {
      for (int i = lane; i < nparts; i += 64) {
        raw += partials[2 * i];
        act += partials[2 * i + 1];
      }
      raw = wave_sum_u64(raw);
      act = wave_sum_u64(act);
    }
    if (lane == 0) {
      put(0, (uint32_t)raw);
      put(1, (uint32_t)(raw >> 32));
      put(2, (uint32_t)act);
      put(3, (uint32_t)(act >> 32));
      put(4, (uint32_t)committed);
      put(5, (uint32_t)chosen);
      put(6, running);
      put(7, running < (unsigned)max_overlaps ? running : (unsigned)max_overlaps);
    }
  }
}

}  // namespace ffn
