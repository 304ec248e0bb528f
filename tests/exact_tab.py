"""Table-form row maps (include/vtx.h: physical row = base + m + tab[m // grp]) for the exact tests; importable without a GPU.

A TabLayout describes one table-mapped buffer the way vtx/functions.py::_compaction_plan builds it for the DropPath-compacted
FFN: `kept` of `n_units` clips of `grp` rows each, group j of the compact problem = the j-th kept clip, tab[j] = (kept[j] - j) * grp,
plus the spare entry the GEMM tile maps read.  It gives the table, the `max_step` argument of ops.tabmap, the CPU index vector
every reference gathers / scatters through, and the complementary layout of the dropped clips over the same buffer.

Every buffer has at least base + M + n_groups * max_step + 1 rows (for the kept AND the dropped table) plus a sentinel tail: a
kernel that applies the closed form (grp, skip = max_step, base) instead of the table stays inside the allocation and fails by
comparison.

The GEMM / copy cases below are built on tests/exact.py (integer operands, dyadic scales: the correct output is unique) and are
compared with equality; tests/test_exact_tab_premise.py asserts their premises on the CPU.
"""
import functools

import torch

import exact as X

N_UNITS = 9
TAIL = 3                                        # sentinel rows behind the bound
# kept clips out of 9: steps of 2, 0 and 3 groups with tab[0] = 0; first clip dropped (tab[0] != 0); a single group (one entry
# plus the spare); only the last dropped (the table is all zeros)
KEPT = ((0, 3, 4, 8), (2, 3, 7), (5,), (0, 1, 2, 3, 4, 5, 6, 7))
# what a table CANNOT be told from a closed form on: one group has no step, an all-zero table is skip = 0
DEGENERATE = ((5,), (0, 1, 2, 3, 4, 5, 6, 7))
# 256: every boundary on a tile boundary, the smallest grp of the fast tile map; 257: the boundary drifts one row per group through
# the tile (TimeSformer's 1 + 16 * 16); 300: boundaries inside 16-row epilogue passes; 44: several boundaries per tile (map_row)
GROUPS = (256, 257, 300, 44)
GROUPS_FAST = (256, 257, 300)


def table_of(idx, grp):
    """The int32 table of _compaction_plan: one offset per group + the spare entry (equal to the last)."""
    t = [(c - j) * grp for j, c in enumerate(idx)]
    return t + [t[-1] if t else 0]


def max_step_of(tab):
    return max([b - a for a, b in zip(tab, tab[1:])] + [0])


def _bound(idx, grp, base):
    """Rows a buffer needs so that the closed form (grp, max_step, base) of this table stays inside it."""
    return base + len(idx) * grp + len(idx) * max_step_of(table_of(idx, grp)) + 1


class TabLayout:
    def __init__(self, grp, kept, n_units=N_UNITS, base=0):
        kept = tuple(kept)
        assert kept and list(kept) == sorted(set(kept)) and 0 <= kept[0] and kept[-1] < n_units
        self.grp, self.kept, self.n_units, self.base = grp, kept, n_units, base
        self.complement = tuple(i for i in range(n_units) if i not in kept)
        self.n_groups = len(kept)
        self.M = self.n_groups * grp
        self.tab = table_of(kept, grp)
        self.max_step = max_step_of(self.tab)
        m = torch.arange(self.M)
        self.rows = base + m + torch.tensor(self.tab)[m // grp]
        self.bound = max(_bound(kept, grp, base), _bound(self.complement, grp, base), base + n_units * grp)
        self.phys = self.bound + TAIL
        self._dev = None

    def dropped(self):
        """The layout of the other clips over the same buffer (the drop table of _compaction_plan)."""
        assert self.complement
        d = TabLayout(self.grp, self.complement, self.n_units, self.base)
        assert d.phys == self.phys
        return d

    def closed_rows(self, skip):
        """Index vector of the closed form (grp, skip, base): what a kernel that ignores the table addresses."""
        m = torch.arange(self.M)
        return self.base + m + (m // self.grp) * skip

    def boundaries(self):
        """Logical rows at which a new group starts (without row 0)."""
        return [j * self.grp for j in range(1, self.n_groups)]

    def unmapped(self):
        um = torch.ones(self.phys, dtype=torch.bool)
        um[self.rows] = False
        return um

    def rowmap(self, ops):
        """ops.tabmap over the uploaded table (kept alive by this object: the map holds a raw device pointer)."""
        if self._dev is None:
            self._dev = ops.upload_i32(self.tab, torch.device('cuda', torch.cuda.current_device()))
        m = ops.tabmap(self.grp, self._dev, self.max_step)
        m.base = self.base
        return m

    def __repr__(self):
        return f'tab(grp={self.grp}, kept={list(self.kept)}/{self.n_units}, base={self.base})'


@functools.lru_cache(maxsize=None)
def layout(grp, kept, base=0):
    return TabLayout(grp, kept, N_UNITS, base)


def base_of(grp, kept):
    """Base of the layouts the GPU file uses: 0 for grp 256 (boundaries stay on tile boundaries of the buffer too), else a few rows."""
    return 0 if grp == 256 else 1 + len(kept)


def all_layouts():
    """Every kept layout the GPU file uses; their .dropped() are the drop layouts."""
    return [layout(grp, kept, base_of(grp, kept)) for grp in GROUPS for kept in KEPT]


# ------------------------------------------------------------------------------------------------- vtx_gemm_nt
GEMM_N, GEMM_K = 320, 192
# cmap a table with bias; cmap = rmap the same table; table C with a closed-form R over a compact buffer, and the reverse (a kernel
# that uses one map for both fails); table + residual + row_scale, rs = (grp, 1, 1, 0): the fc2 call of FFNFn._forward_compact
GEMM_EPILOGUES = ('bias', 'res_same', 'ctab_rclosed', 'cclosed_rtab', 'fc2')
CLOSED = (97, 2, 3)                             # (grp, skip, base) of the closed-form map of the mixed cases


class ClosedLayout:
    """Closed-form map over a compact buffer of its own (the other side of the mixed cases)."""

    def __init__(self, M, grp=CLOSED[0], skip=CLOSED[1], base=CLOSED[2]):
        self.M, self.grp, self.skip, self.base = M, grp, skip, base
        m = torch.arange(M)
        self.rows = base + m + (m // grp) * skip
        self.phys = int(self.rows[-1]) + 1 + TAIL

    def unmapped(self):
        um = torch.ones(self.phys, dtype=torch.bool)
        um[self.rows] = False
        return um

    def rowmap(self, ops):
        return ops.rowmap(self.grp, self.skip, self.base)


def junk(shape, seed):
    """Non-zero integers for the rows / columns a kernel must not read."""
    return X.ints(shape, 1, 5, 1.0, seed + 977) * 7.0


@functools.lru_cache(maxsize=None)
def gemm_case(grp, kept, epi, K=GEMM_K, N=GEMM_N):
    """One vtx_gemm_nt case on a table layout as CPU float32 tensors and the float64 expected result [M, N] in logical row order.
    Keys: lay (TabLayout of the table side), A [M, K], W, bias, R (physical buffer of the residual, junk outside its map) or None,
    rlay / clay (the layout objects R is read / C is written through), scale ([n_groups]) or None, expected, kind."""
    lay = layout(grp, kept, base_of(grp, kept))
    M = lay.M
    seed = 1000 * grp + 10 * len(kept) + kept[0] + K
    A, W, bias = X.nt_operands(M, N, K, 'round', seed)
    c = dict(lay=lay, M=M, N=N, K=K, A=A, W=W, bias=bias, R=None, rlay=None, clay=lay, scale=None, kind='round', epi=epi)
    name = f'tab gemm {epi} grp={grp} kept={list(kept)} K={K}'
    if epi == 'bias':
        c['expected'] = X.nt_reference(name, A, W, bias=bias)
        return c
    closed = ClosedLayout(M)
    c['rlay'] = closed if epi == 'ctab_rclosed' else lay
    c['clay'] = closed if epi == 'cclosed_rtab' else lay
    Rl = X.ints((M, N), -32, 32, 1.0, seed + 6)                  # residual in logical row order
    R = junk((c['rlay'].phys, N), seed + 7)
    R[c['rlay'].rows] = Rl
    c['R'] = R
    if epi == 'fc2':
        # (no 2.0: (512 + ..) * 2 + integer residuals lies where the bf16 spacing is 8 -- 1/8 ties, below the rounding premise)
        c['scale'] = X.dyadic_scales(lay.n_groups, seed + 4, choices=(0.5, 1.0))
        c['scale'][0] = 0.5
        c['scale'][-1] = 1.0 if lay.n_groups > 1 else 0.5
        c['expected'] = X.nt_reference(name, A, W, bias=bias, scale=c['scale'].repeat_interleave(grp), R=Rl)
    else:
        c['expected'] = X.nt_reference(name, A, W, bias=bias, R=Rl)
    return c


def gemm_cases(groups=GROUPS):
    """(grp, kept, epi, K) of every GEMM case; K = 128 (two K tiles: the persistent kernel's minimum) once per group size."""
    out = [(grp, kept, epi, GEMM_K) for grp in groups for kept in KEPT for epi in GEMM_EPILOGUES]
    out += [(grp, KEPT[0], epi, 128) for grp in groups for epi in ('bias', 'fc2')]
    return out


# ------------------------------------------------------------------------------------------------- LayerNorm
# exact_ln.fwd_case / bwd_case at rows = n_kept * grp, seeded as the LayerNorm file seeds its own (exact_ln.case_seed)
LN_D = (128, 200, 768, 1024)                    # ragged / two chunks / the benchmark's width / the widest float32-stream row
LN_D_WIDE = (1280,)                             # vtx_layernorm_fwd only: D > 1024 takes one row per trip whatever ln_rows says
LN_FWD_KINDS = ('f32', 'bf16')
LN_ACC_KINDS = ('acc', 'acc0')
LN_BWD_KINDS = ('f32', 'bf16', 'x32', 'g32')


def ln_rows_of(grp):
    """Row counts of the LayerNorm cases of one group size (one per kept pattern)."""
    return sorted({len(kept) * grp for kept in KEPT})


# ------------------------------------------------------------------------------------------------- copies and fix-ups
COPY_D = 136                                    # 17 column chunks of 8: no power of two
FIX_GROUP = 4                                   # group_rows of the dropped-row kernels (257 % 4 != 0: a ragged last group)


@functools.lru_cache(maxsize=None)
def copy_case(grp, kept):
    """Integer data of the copy / fix-up cases on one layout: src (physical, every row distinct and non-zero), per-group dyadic
    scales, a bias, the scales (with zeros) of the dropped-row kernels."""
    lay = layout(grp, kept, base_of(grp, kept))
    seed = 7000 + grp + len(kept)
    src = X.ints((lay.phys, COPY_D), 1, 16, 1.0, seed) * (X.ints((lay.phys, COPY_D), 0, 1, 1.0, seed + 1) * 2 - 1)
    scale = X.dyadic_scales(lay.n_groups, seed + 2, choices=(0.5, 1.0, 2.0))
    bias = X.ints((COPY_D,), -8, 8, 1.0, seed + 3)
    ng = (lay.M + FIX_GROUP - 1) // FIX_GROUP
    s = X.dyadic_scales(ng, seed + 4)
    s[0], s[-1] = 0.0, 0.0                                       # the first and the (possibly ragged) last group are dropped
    s[1] = 1.0
    return dict(lay=lay, src=src, scale=scale, bias=bias, s=s)


def copy_expected(c):
    """float64 expected values of the copy / fix-up kernels, in logical row order of the kept (resp. dropped) layout."""
    lay = c['lay']
    src = c['src'].double()
    out = dict(gather=src[lay.rows] * c['scale'].double().repeat_interleave(lay.grp)[:, None])
    drop = (c['s'] == 0).repeat_interleave(FIX_GROUP)[:lay.M]
    out['drop'] = drop
    out['fix'] = src[lay.rows] + c['bias'].double()
    out['colsum'] = src[lay.rows][drop].sum(0)
    return out
