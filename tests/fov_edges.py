"""FoV geometries at which a rule of conv_caps (ffn_amd/csrc/ffn_stack_plan.h) is at its
limit, one list for the CPU tests (tests/test_stack_plan.py) and the GPU tests
(tests/test_gpu_fov_edges.py).  Not a test.  tools/fov_edges.py is the sweep that found
them: re-run it when a row budget or a chunk size changes.

EDGES: (name, fov_zyx, deltas_zyx, what it is there for).  Models take xyz: reverse the
triples for ConvStack3DFFNModel.  FACTS[name]: the stated property, in the vocabulary of
test_stack_plan._edge_facts (all for depth >= 2; a slack is budget minus need, in LDS
rows: 0 is exactly inside, negative is a miss)."""


def _quarter(fov):
  return tuple((f - 1) // 4 for f in fov)


def _e(name, fov, what, deltas=None):
  return (name, tuple(fov), tuple(deltas) if deltas else _quarter(fov), what)


EDGES = [
    _e('m_rows_exact', (45, 5, 25), 'default 8; conv32m span + halo = kMRows exactly'),
    _e('m_rows_miss', (35, 35, 35), 'default 6: the 96-voxel form misses by 1 row, conv32m '
       'by 2; variants 7, 8, 9, 10 refuse'),
    _e('d_rows_miss', (35, 35, 51), 'default 0: Rc_k raw 322 > 320, Rc = 320; variants 2, '
       '6 .. 10 refuse'),
    _e('ks10_small', (19, 3, 3), 'Rc_k = 320 (KS 10), 2 chunks, default 8'),
    _e('ks10_large', (35, 37, 49), 'Rc_k = 320 (raw 316), default 6, exact_variant 0'),
    _e('ks9_exact', (13, 5, 29), 'Rc_k raw = 288, no rounding slack'),
    _e('e_rows_tight', (7, 3, 25), '96-voxel form 2 rows inside, conv32m 1 row inside'),
    _e('perm021_resident', (29, 29, 39), 'oa (0,2,1), default 9, n_tail = 1 (31 voxels), '
       'n_tail3 = 1'),
    _e('perm021_tail7', (25, 23, 57), 'oa (0,2,1), default 9, n_tail = 1 with 7 voxels, '
       'exact_variant 0'),
    _e('tail_256', (37, 41, 27), 'identity layout, default 9, n_tail = 256 (the cap), '
       'n_tail3 = 86, n_half = 512'),
    _e('tail_258', (21, 63, 31), 'n_tail would be 258: t_ok false, default 8 with 321 '
       'chunks; 9 and 10 refuse'),
    _e('m_256', (39, 31, 27), 'nchunks_m = 256 exactly, last chunk 3 voxels; default 8; 9 '
       'refuses'),
    _e('last_one', (5, 7, 11), 'V = 1 mod 128: a last conv32m chunk of one voxel; 3 conv32d '
       'chunks'),
    _e('two_chunks', (3, 5, 11), 'nchunks_m = nchunks_k = 2, the least the split-product '
       'kernels admit'),
    _e('one_chunk_5', (5, 5, 5), 'default 2; every fp16 variant refuses; less than one '
       'chunk of any kernel'),
    _e('one_chunk_3', (3, 3, 3), 'default 2; every fp16 variant refuses; less than one '
       'chunk of any kernel'),
    _e('perm021_small', (13, 9, 41), 'oa (0,2,1), default 8, three different deltas: for '
       'the canvas step', deltas=(3, 2, 10)),
    _e('perm120_small', (9, 13, 41), 'the same voxels under (1,2,0), as its control',
       deltas=(2, 3, 10)),
    _e('perm102_small', (73, 3, 3), 'oa (1,0,2), default 8: the smallest FoV that chooses '
       'that row of kPerms (none with fz, fy <= 65 does)', deltas=(18, 1, 1)),
    _e('widest', (3, 3, 131), 'lds_bytes = 163,584 <= 160 KB: the widest row conv32 stages; '
       'oa (0,2,1), default 8, exact_variant 0', deltas=(0, 0, 32)),
]

# ffn_engine_create must refuse it (FFN_ERR_ARG): conv32's three staged rows pass 160 KB
TOO_WIDE = ('too_wide', (3, 3, 133), (0, 0, 33), 'lds_bytes = 165,120 > 160 KB')

FACTS = {
    'm_rows_exact': dict(default=8, m_slack=0),
    'm_rows_miss': dict(default=6, oa=(0, 1, 2), m_slack=-2, e_slack=-1),
    'd_rows_miss': dict(default=0, exact=0, rck_raw=322, Rc=320),
    'ks10_small': dict(default=8, Rc_k=320, nchunks_k=2),
    'ks10_large': dict(default=6, exact=0, Rc_k=320, rck_raw=316),
    'ks9_exact': dict(Rc_k=288, rck_raw=288),
    'e_rows_tight': dict(e_slack=2, m_slack=1),
    'perm021_resident': dict(default=9, oa=(0, 2, 1), n_tail=1, tail_voxels=31, n_tail3=1),
    'perm021_tail7': dict(default=9, exact=0, oa=(0, 2, 1), n_tail=1, tail_voxels=7),
    'tail_256': dict(default=9, oa=(0, 1, 2), n_tail=256, n_tail3=86, n_half=512),
    'tail_258': dict(default=8, n_tail=258, nchunks_m=321),
    'm_256': dict(default=8, nchunks_m=256, last_m=3),
    'last_one': dict(default=8, last_m=1, nchunks_k=3),
    'two_chunks': dict(nchunks_m=2, nchunks_k=2),
    'one_chunk_5': dict(default=2, nchunks_m=1, nchunks_k=1),
    'one_chunk_3': dict(default=2, nchunks_m=1, nchunks_k=1),
    'perm021_small': dict(default=8, oa=(0, 2, 1)),
    'perm120_small': dict(default=8, oa=(1, 2, 0)),
    'perm102_small': dict(default=8, oa=(1, 0, 2)),
    'widest': dict(default=8, exact=0, oa=(0, 2, 1), lds_bytes=163584),
    'too_wide': dict(lds_bytes=165120),
}

BY_NAME = {e[0]: e for e in EDGES + [TOO_WIDE]}
