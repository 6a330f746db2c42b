// TEST INFRASTRUCTURE: a stand-alone program that drives the library's seed loop
// (tests/seed_loop_shim.cpp -> ffn_host::SeedLoop) over a stub device kept in plain
// arrays, for a build with -fsanitize=address,undefined (tests/test_seed_loop.py
// builds and runs it).  One call per segment, a voided step with its resume, a
// seed listed twice, one whose FoV leaves the canvas, a list longer than a window.
#include <cmath>
#include <cstdio>

#include "seed_loop_shim.cpp"

namespace {

const int N = 24, M = 2;  // canvas edge, FoV margin
std::vector<float> g_seed(N* N* N, NAN);
std::vector<int32_t> g_seg(N* N* N, 0);
int g_steps = 0, g_void_at = 5;

size_t at(int z, int y, int x) { return ((size_t)z * N + y) * N + x; }
bool inside(const int32_t* p) {
  return p[0] >= 0 && p[0] < N && p[1] >= 0 && p[1] < N && p[2] >= 0 && p[2] < N;
}

int stub_step(const ffn_step_request* rq, const ffn_step_params*, ffn_step_result* res) {
  if (g_steps == g_void_at) {
    g_void_at = -1;
    return FFN_ERR_RANGE;  // once: nothing pasted
  }
  ++g_steps;
  std::memset(res, 0, sizeof(*res));
  const int32_t* p = rq->pos;
  for (int z = p[0] - M; z <= p[0] + M; ++z)
    for (int y = p[1] - M; y <= p[1] + M; ++y)
      for (int x = p[2] - M; x <= p[2] + M; ++x) g_seed[at(z, y, x)] = 2.0f;
  // one move along +x while the FoV stays inside, the other faces below threshold
  for (int k = 0; k < 6; ++k) res->face_score[k] = -5.0f;
  res->face_score[5] = 3.0f;
  res->face_index[5] = 1 * 3 + 1;  // the face's centre, deltas (1, 1, 1)
  const int32_t q[3] = {p[0], p[1], p[2] + 1};
  res->face_seg[5] = inside(q) ? g_seg[at(q[0], q[1], q[2])] : 0;
  res->start_logit = g_seed[at(rq->start_pos[0], rq->start_pos[1], rq->start_pos[2])];
  for (int k = 0; k < rq->num_candidates; ++k) {
    const int32_t* c = rq->candidates[k];
    res->cand_seed[k] = inside(c) ? g_seed[at(c[0], c[1], c[2])] : NAN;
    res->cand_seg[k] = inside(c) ? g_seg[at(c[0], c[1], c[2])] : 0;
  }
  return FFN_OK;
}

int stub_read(const int32_t* p, float* seed, int32_t* seg) {
  *seed = inside(p) ? g_seed[at(p[0], p[1], p[2])] : NAN;
  *seg = inside(p) ? g_seg[at(p[0], p[1], p[2])] : 0;
  return FFN_OK;
}

int stub_turn(const ffn_turn_request* rq, const int32_t* cand, ffn_turn_result* out,
              int32_t max_overlaps, int32_t*, int64_t*, int32_t* flags, float* cseed,
              int32_t* cseg) {
  (void)max_overlaps;
  std::memset(out, 0, sizeof(*out));
  out->chosen = -1;
  if (rq->do_commit) {
    int64_t actual = 0;
    for (int z = rq->lo[0]; z < rq->hi[0]; ++z)
      for (int y = rq->lo[1]; y < rq->hi[1]; ++y)
        for (int x = rq->lo[2]; x < rq->hi[2]; ++x)
          if (g_seed[at(z, y, x)] >= rq->segment_threshold && g_seg[at(z, y, x)] <= 0)
            ++actual;
    out->counts.raw_segmented_voxels = out->counts.actual_segmented_voxels = actual;
    if (actual >= rq->min_segment_size) {
      out->committed = 1;
      for (int z = rq->lo[0]; z < rq->hi[0]; ++z)
        for (int y = rq->lo[1]; y < rq->hi[1]; ++y)
          for (int x = rq->lo[2]; x < rq->hi[2]; ++x)
            if (g_seed[at(z, y, x)] >= rq->segment_threshold && g_seg[at(z, y, x)] <= 0)
              g_seg[at(z, y, x)] = rq->segment_id;
    }
  }
  int32_t& mk = g_seg[at(rq->mark_pos[0], rq->mark_pos[1], rq->mark_pos[2])];
  if ((rq->mark_mode == 1 || (rq->mark_mode == 2 && !out->committed)) && mk == 0) mk = -1;
  for (int k = 0; k < rq->num_candidates; ++k) {
    const int32_t* p = cand + 3 * k;
    cseed[k] = g_seed[at(p[0], p[1], p[2])];
    cseg[k] = g_seg[at(p[0], p[1], p[2])];
    flags[k] = 3;
    if (out->chosen >= 0) continue;
    if (cseg[k] > 0) {
      flags[k] = 1;
      continue;
    }
    bool close = false;
    for (int z = std::max(p[0] - 1, 0); z <= std::min(p[0] + 1, N - 1); ++z)
      for (int y = std::max(p[1] - 1, 0); y <= std::min(p[1] + 1, N - 1); ++y)
        for (int x = std::max(p[2] - 1, 0); x <= std::min(p[2] + 1, N - 1); ++x)
          close = close || g_seg[at(z, y, x)] > 0;
    if (close) {
      flags[k] = 2;
      g_seg[at(p[0], p[1], p[2])] = -1;
      continue;
    }
    flags[k] = 0;
    out->chosen = k;
    if (rq->do_init) {
      std::fill(g_seed.begin(), g_seed.end(), NAN);
      g_seed[at(p[0], p[1], p[2])] = rq->init_value;
    }
  }
  return FFN_OK;
}

}  // namespace

int main() {
  std::vector<int32_t> seeds;
  auto add = [&](int z, int y, int x) { seeds.insert(seeds.end(), {z, y, x}); };
  add(4, 4, 4);
  add(4, 4, 4);                                   // listed twice
  for (int x = 2; x < 22; ++x) add(4, 4, x);      // more than one window, all refused
  add(12, 12, 23);                                // FoV outside the canvas
  add(12, 12, 3);
  add(19, 19, 10);
  void* st = shim_state_create();
  void* sl = shim_seed_state_create();
  ffn_seed_loop_args a;
  std::memset(&a, 0, sizeof(a));
  a.seeds = seeds.data();
  a.num_seeds = (int64_t)seeds.size() / 3;
  a.segment.step.move_threshold = 1.0f;
  a.segment.step.deleted_threshold = NAN;
  a.segment.score_threshold = 1.0;
  for (int k = 0; k < 3; ++k) {
    a.segment.deltas_zyx[k] = 1;
    a.segment.margin_zyx[k] = M;
    a.segment.shape_zyx[k] = N;
    a.min_boundary_dist[k] = 1;
    a.half_pred[k] = M;
  }
  a.segment.prefetch = 8;
  a.init_value = 2.5f;
  a.segment_threshold = 0.5f;
  a.min_segment_size = 10;
  a.next_segment_id = 1;
  a.turn_candidates = 8;
  a.max_segments = 1;
  std::vector<ffn_seed_record> recs(4);
  std::vector<int32_t> ids(64);
  std::vector<int64_t> counts(64);
  a.records = recs.data();
  a.max_records = (int32_t)recs.size();
  a.overlap_ids = ids.data();
  a.overlap_counts = counts.data();
  a.max_overlaps = 64;
  int committed = 0, calls = 0, voided = 0;
  int64_t steps = 0;
  for (;;) {
    ffn_seed_loop_result r;
    const int rc = shim_segment_all(st, sl, stub_step, stub_read, stub_turn, &a, &r);
    ++calls;
    for (int k = 0; k < r.num_records; ++k) {
      steps += recs[k].segment.num_steps;
      if (recs[k].outcome == FFN_SEED_COMMITTED) {
        ++committed;
        a.max_existing_id = recs[k].segment_id;
        a.next_segment_id = recs[k].segment_id + 1;
      }
    }
    a.first_seed = r.next_seed;
    a.resume = 0;
    if (rc == FFN_ERR_RANGE && r.in_segment) {
      ++voided;
      a.resume = 1;
      continue;
    }
    if (rc != FFN_OK) {
      std::printf("rc %d\n", rc);
      return 1;
    }
    if (r.exhausted) break;
  }
  shim_seed_state_destroy(sl);
  shim_state_destroy(st);
  std::printf("calls %d committed %d steps %lld (device %d) voided %d\n", calls, committed,
              (long long)steps, g_steps, voided);
  return committed == 3 && voided == 1 && steps == g_steps ? 0 : 1;
}
