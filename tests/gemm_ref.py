"""
fp64 reference, derived per-element bounds, input families and an fp32 emulation for every GEMM outside the fused chains:

    dw_kernel<F16|BF16>, dw_split_wide_kernel, dw_reduce_kernel, lin_out_grad_kernel + lin_out_reduce_kernel     (pnr_bwd.hip)
    linear_f32_kernel, wgrad_f32_kernel + wgrad_reduce_f32_kernel, gemm3_kernel<A_KC,B_KC,STAGES>                 (pnr_f32.hip)

Plain numpy on the CPU.  tests/test_gemm_ref_host.py proves the claims made here (no GPU); tests/test_hip_gemm_sweep.py holds the
kernels to them; profiles/gemm_sweep_notes.md has the measured figures.

REFERENCE.  Every product is written reduction-last:  C[i][j] = sum_k A[i][k] B[j][k].  The operands are EXACTLY the values the
kernel is given -- 16-bit values and fp32 values as they are, (head, tail) pairs as they are; for gemm3_kernel, which splits fp32
operands itself, the pairs are this module's restatement of g3_split4 (f16_split: h = f16(v s) saturated at +-65504,
l = f16(v s - h)).  `product` / `product_split` return, per element and in float64 (whose own error, K 2^-53 S, is 2^-30 of
the bounds below):

    value   what the kernel is DEFINED to compute; for the split forms sum(ah bh + ah bl + al bh), the dropped al bl left out
    S       sum |a| |b|   (|a| = |ah| + |al| for a pair)
    drop    sum |al bl|   (zero for the plain forms)

DERIVED BOUND (`finish`).  Nothing here is fitted to a kernel.  u = 2^-23, NOT 2^-24: the f16 matrix instruction's sum rounds
toward -inf (profiles/mlp_backward_stage_notes.md), and a directed rounding loses up to one whole last place.

    accumulation   A sum of n terms formed in ANY order by n - 1 roundings of relative size <= u is off by at most
                   ((1 + u)^(n-1) - 1) sum|term| <= gamma(n) S,  gamma(n) = n u / (1 - n u).  n_add = (kept products per k) x
                   (reduction length) + (slices of a split reduction) + (epilogue operations).  A matrix instruction that
                   aligns its 16 products to the largest exponent and truncates is covered term by term: each product loses
                   < one last place of a number <= the sum of magnitudes.
    products       + u S where a product is not exact in fp32: fp32 x fp32 (linear_f32_kernel, wgrad_f32_kernel) and
                   fp32 x 16-bit (lin_out_grad_kernel).  16-bit x 16-bit products have <= 22 significant bits: exact.
    epilogue       every scaling / bias / residual operation rounds once: n_epi u (|result| + |bias| + |Yin|).
    subnormal      a sum that lands below 2^-126 may be flushed: n_add 2^-126 (not where S = 0: a sum of zeros is zero).  Where THIS module makes the split (f16_split),
                   a tail below 2^-14 is an f16 subnormal with step 2^-24; the bound needs no term for it because the
                   reference multiplies the very pairs the split yields (test_hip_gemm_sweep.py would show a device split that
                   differs) -- the step enters the CONTRACT budget below, where the caller's fp32 value is the yardstick.

CONTRACT (`contract_bound`).  Against the plain fp64 product of the caller's fp32 values the project promises 2e-5 (split forms)
and 2e-6 (exact forms) of the tensor's scale (tests/test_hip_composed.py).  Per element that reads
|err| <= tol max(|ref|, floor).  The floor first proposed, S 2^-22, does not hold up: on a cancelling element |ref| << S, and the
error that is ALLOWED there is the whole budget
        derived bound + sum|al bl| (dropped, <= 2^-22 S) + sum(|da| |b| + |a| |db| + |da| |db|)   (da = a - ah - al: <= 2^-22 |a|, or the
                                                                                       2^-25 half-step of a subnormal tail)
which is of order n_add u S, i.e. (n_add 2^-23 / tol) S -- several S at tol = 2e-5 and n = 1000.  The floor is therefore that
budget itself: contract_bound = max(tol |ref|, budget), with the budget computed exactly from the operands.

FAMILIES.
    exact       every partial sum in every legal order is exactly representable in fp32, so the device must return the
                reference BIT FOR BIT.  Plain forms: integers |v| <= amax, amax = min(cap, floor(sqrt((2^24 - 1) / n))) with
                cap 8 (f16, fp32) or 256 (bf16: 8 significant bits) -- all terms are integers and S <= n amax^2 < 2^24.
                Split forms: v = h + t 2^-12 with h an integer, 1 <= |h| <= A, t in {-1, 0, 1}, or v = 0.  |t 2^-12| is below
                half a last place of any |h| >= 1 (f16: 2^-11), so the split returns exactly (h, t 2^-12); the kept products
                are integers (h h') and multiples of 2^-12 (h t'), the dropped one a multiple of 2^-24: every partial sum is
                a multiple of 2^-12 below 2^12 when n (A^2 + 2 A 2^-12) < 2^12, i.e. A = floor(sqrt(4000 / n)) (capped at 8):
                24 bits.  Power-of-two scales (the gradient scale, out_scale) and integer bias / residual keep that.
                Every element is a function of (row, column) modulo small primes: a wrong row, column, permutation entry or
                slice changes the sums.
    ranged      iid normal x a per-column scale 2^-12 .. 2^4, about half the entries zeroed, a few columns all-zero: the
                matching outputs must be exactly 0.0, everything else inside the derived bound.
    cancelling  pairs (v, -v (1 + eps)) along the reduction: |ref| << S, only a magnitude-based bound means anything.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -23          # unit roundoff of a DIRECTED fp32 rounding
FTZ = 2.0 ** -126       # smallest normal fp32: what a flushed sum can lose
F16_MAX = 65504.0

Ref = namedtuple("Ref", "value S drop")


def gamma(n):
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------------ number formats
def f16_split(v, scale=1.0):
    """g3_split4 under FP16_OVFL: fp32 v (times the power-of-two scale) -> (head, tail) float16 arrays."""
    p = np.asarray(v, np.float32) * np.float32(scale)
    h = np.clip(p, -F16_MAX, F16_MAX).astype(np.float16)
    l = np.clip(p - h.astype(np.float32), -F16_MAX, F16_MAX).astype(np.float16)
    return h, l


def to_bf16(v):
    """fp32 -> nearest-even bfloat16, returned as the float32 that holds it."""
    b = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def trunc_bf16(v):
    """fp32 -> bfloat16 by dropping the low 16 bits (the mutation 'operand truncated to bf16')."""
    return (np.asarray(v, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


# ------------------------------------------------------------------------------------------------ reference
def product(A, B):
    """A (m,K), B (n,K): the operand values as given -> Ref of C = A B^T in float64."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return Ref(A @ B.T, np.abs(A) @ np.abs(B).T, np.zeros((A.shape[0], B.shape[0])))


def product_split(Ah, Al, Bh, Bl):
    """(head, tail) operands -> Ref of the three KEPT products; drop = sum |al bl|."""
    Ah, Al, Bh, Bl = (np.asarray(x, np.float64) for x in (Ah, Al, Bh, Bl))
    value = Ah @ Bh.T + Ah @ Bl.T + Al @ Bh.T
    S = (np.abs(Ah) + np.abs(Al)) @ (np.abs(Bh) + np.abs(Bl)).T
    return Ref(value, S, np.abs(Al) @ np.abs(Bl).T)


def split_residual(A, Ah, Al, B, Bh, Bl):
    """sum(|da| |b| + |a| |db| + |da| |db|) >= |a b - (ah + al)(bh + bl)|: what the pairs themselves miss of the fp32 values A, B
    they were split from (the second-order term counts where both operands are f16 subnormals and da / a is not small)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    dA = np.abs(A - np.asarray(Ah, np.float64) - np.asarray(Al, np.float64))
    dB = np.abs(B - np.asarray(Bh, np.float64) - np.asarray(Bl, np.float64))
    return dA @ np.abs(B).T + np.abs(A) @ dB.T + dA @ dB.T


def finish(ref, n_red, n_slices=1, terms=1, rounded=False, out_scale=1.0, n_scale_ops=0, bias=None, yin=None, keep=None):
    """The epilogue of every form and the DERIVED per-element bound (module docstring).
    result = keep ? ref.value * out_scale + bias : 0, + yin.   -> (value, bound), float64.
    n_red: reduction length; terms: kept products per k (3 for the split forms); n_slices: partial sums of a split reduction;
    n_scale_ops: roundings spent on out_scale (0 when it is a power of two or absent); bias (n,) / yin (m,n) / keep (m,n) bool."""
    n_epi = n_scale_ops + (bias is not None) + (yin is not None)
    n_add = terms * n_red + n_slices + n_epi
    sc = abs(float(out_scale))
    value = ref.value * float(out_scale)
    mag = np.abs(value)
    if bias is not None:
        value = value + np.asarray(bias, np.float64)[None, :]
        mag = mag + np.abs(np.asarray(bias, np.float64))[None, :]
    bound = (gamma(n_add) + (U if rounded else 0.0)) * ref.S * sc + n_add * FTZ * max(sc, 1.0) * (ref.S > 0)  # S == 0: exactly zero
    if keep is not None:
        value, bound, mag = np.where(keep, value, 0.0), np.where(keep, bound, 0.0), np.where(keep, mag, 0.0)
    if yin is not None:
        value = value + np.asarray(yin, np.float64)
        mag = mag + np.abs(np.asarray(yin, np.float64))
    live = 1.0 if keep is None else keep.astype(np.float64)
    return value, bound + n_epi * U * (np.abs(value) + mag) * live


def contract_bound(plain, tol, derived, drop=0.0, residual=0.0, out_scale=1.0):
    """|device - plain fp64 product of the caller's values| <= max(tol |plain|, budget); budget = derived bound + what the split drops."""
    budget = derived + (np.asarray(drop) + np.asarray(residual)) * abs(float(out_scale))
    return np.maximum(tol * np.abs(plain), budget)


def worst_ratio(got, value, bound):
    """max over elements of |got - value| / bound (0/0 counts as 0, x/0 as inf): the number the notes record."""
    err = np.abs(np.asarray(got, np.float64) - value)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ families
def _grid(rows, cols):
    return np.arange(rows, dtype=np.int64)[:, None], np.arange(cols, dtype=np.int64)[None, :]


def exact_amax(n_red, cap=8):
    """largest integer amplitude with n_red amax^2 < 2^24 (plain forms)."""
    return int(max(1, min(cap, np.floor(np.sqrt((2.0 ** 24 - 1) / max(n_red, 1))))))


def exact_ints(rows, cols, n_red, seed=0, cap=8):
    """(rows, cols) float32 integers in [-amax, amax], a function of (row, column) modulo small primes."""
    a = exact_amax(n_red, cap)
    r, c = _grid(rows, cols)
    v = ((r % 251) * 3 + (c % 241) * 5 + (r % 7) * (c % 11) + (r % 13) * (c % 5) + 7 * seed) % (2 * a + 1) - a
    return v.astype(np.float32)


def exact_split(rows, cols, n_red, seed=0):
    """(rows, cols) float32 v = h + t 2^-12 (or 0): the split-form exact family of the module docstring."""
    A = int(max(1, min(8, np.floor(np.sqrt(4000.0 / max(n_red, 1))))))
    assert n_red * (A * A + 2 * A * 2.0 ** -12) < 2.0 ** 12, "exact_split: reduction too long to stay exact"
    r, c = _grid(rows, cols)
    k = ((r % 251) * 3 + (c % 241) * 5 + (r % 7) * (c % 11) + (r % 13) * (c % 5) + 7 * seed) % (2 * A + 1) - A
    t = ((r % 5) * 2 + (c % 7) * 3 + (r % 3) * (c % 2) + seed) % 3 - 1
    v = np.where(k == 0, 0.0, k + t * 2.0 ** -12)
    return v.astype(np.float32)


def ranged(rows, cols, seed=0, zero_cols=(), lo=-12, hi=4):
    """iid normal x per-column 2^lo..2^hi, ~half the entries zero, `zero_cols` all-zero."""
    g = np.random.default_rng(1000 + seed)
    v = g.standard_normal((rows, cols)) * 2.0 ** g.integers(lo, hi + 1, size=(1, cols))
    v = np.where(g.random((rows, cols)) < 0.5, 0.0, v)
    for c in zero_cols:
        if c < cols:
            v[:, c] = 0.0
    return v.astype(np.float32)


def cancelling(rows, cols, seed=0, eps=2.0 ** -9, along=0, flip=True):
    """pairs (v, -v (1 + eps)) along axis `along` (flip=False: pairs (v, v), the other operand of such a product)."""
    g = np.random.default_rng(2000 + seed)
    shape = ((rows + 1) // 2, cols) if along == 0 else (rows, (cols + 1) // 2)
    base = g.standard_normal(shape)
    v = np.repeat(base, 2, axis=along)[:rows, :cols]
    if flip:
        idx = np.arange(v.shape[along]) % 2 == 1
        f = np.where(idx, -(1.0 + eps), 1.0)
        v = v * (f[:, None] if along == 0 else f[None, :])
    return v.astype(np.float32)


def host_perm(n, seed=5):
    """a fixed permutation for the host tests (storage position e -> feature perm[e]); the GPU tests take pnr_storage_perm's."""
    return np.random.default_rng(seed).permutation(n)


def scatter_perm(dW, db, perm, rows_st, cols_st):
    """storage -> feature order as dw_reduce_kernel writes it: out[perm[e]] = raw[e] along the flagged axes."""
    if rows_st:
        o = np.empty_like(dW); o[perm] = dW; dW = o
        if db is not None:
            b = np.empty_like(db); b[perm] = db; db = b
    if cols_st:
        o = np.empty_like(dW); o[:, perm] = dW; dW = o
    return dW, db


# ------------------------------------------------------------------------------------------------ fp32 emulation
def _round_down(x64):
    r = x64.astype(np.float32)
    return np.where(r.astype(np.float64) > x64, np.nextafter(r, np.float32(-np.inf)), r).astype(np.float32)


def _round_near(x64):
    return x64.astype(np.float32)


def emu_sum(terms, bounds, order):
    """fp32 emulation of sum_k over the (A (m,K), B (n,K)) float32 pairs in `terms`, the reduction cut at `bounds`
    (list of (k0, k1) slices, each summed from 0, the partial sums added up afterwards in list order).
    order 0: one product at a time, ascending k, round-to-nearest.
    order 1: blocks of 16 k summed as a pairwise tree and added to the accumulator, descending k inside a block, slices added in
             reverse, every rounding toward -inf (the f16 matrix instruction's direction).
    Products are rounded to fp32 once (exact for 16-bit operands).  -> (m,n) float32 partial sums per slice, and their sum."""
    rnd = _round_near if order == 0 else _round_down
    m, n = terms[0][0].shape[0], terms[0][1].shape[0]
    parts = []
    for k0, k1 in bounds:
        acc = np.zeros((m, n), np.float32)
        if order == 0:
            for k in range(k0, k1):
                for A, B in terms:
                    p = rnd(np.outer(A[:, k].astype(np.float64), B[:, k].astype(np.float64)))
                    acc = rnd(acc.astype(np.float64) + p)
        else:
            for A, B in terms:
                for b0 in range(k0, k1, 16):
                    ps = [rnd(np.outer(A[:, k].astype(np.float64), B[:, k].astype(np.float64))) for k in range(min(b0 + 16, k1) - 1, b0 - 1, -1)]
                    while len(ps) > 1:
                        ps = [rnd(ps[i].astype(np.float64) + ps[i + 1]) if i + 1 < len(ps) else ps[i] for i in range(0, len(ps), 2)]
                    acc = rnd(acc.astype(np.float64) + ps[0])
        parts.append(acc)
    total = np.zeros((m, n), np.float32)
    for p in (parts if order == 0 else parts[::-1]):
        total = rnd(total.astype(np.float64) + p)
    return parts, total


def slices_of(rows, nsplit, slab=32):
    """the row slices every split-K form here uses: ceil(rows / nsplit) rounded up to the slab; trailing slices may be empty."""
    per = -(-rows // nsplit)
    per = -(-per // slab) * slab
    return [(min(z * per, rows), min(z * per + per, rows)) for z in range(nsplit)]


def emu_weight_grad(dY, X, nsplit, order, cls="exact", out_scale=1.0, relu_x=False, perm=None, rows_st=False, cols_st=False,
                    mut=None, stale=None):
    """fp32 emulation of a weight gradient dW = out_scale dY^T [relu]X, db = out_scale sum_rows dY in the arithmetic class `cls`:
        "exact"    exact products + fp32 accumulation   (dY, X: float32 arrays holding 16-bit values; rows beyond `rows` are guard)
        "rounded"  products rounded to fp32             (dY, X: float32)
        "split"    three kept products of (head, tail)  (dY, X: tuples (h, l))
    dY / X carry ONE guard row behind the `rows` that count (shape rows + 1).  `mut` names one of the mutations of
    tests/test_gemm_ref_host.py; `stale` = partial sums (dW parts, db parts) of an earlier call for mut == "stale_slice"."""
    split = cls == "split"
    rows = (dY[0] if split else dY).shape[0] - 1
    pairs = lambda op: tuple(np.asarray(x, np.float32) for x in op) if split else (np.asarray(op, np.float32),)
    ys, xs = pairs(dY), pairs(X)
    if relu_x and mut != "no_relu":
        xs = (np.maximum(xs[0], 0),) + tuple(np.where(xs[0] > 0, x, 0) for x in xs[1:])  # a pair follows its head's sign (split of relu(v))
    n_rows = rows + 1 if mut == "row_beyond" else rows
    bounds = slices_of(rows, nsplit)
    if mut == "drop_tail_slab":
        bounds = [(a, b - (b - a) % 32) for a, b in bounds]
    if mut == "row_beyond":
        last = max(z for z, (a, b) in enumerate(bounds) if b > a)
        bounds[last] = (bounds[last][0], n_rows)
    At = [y.T for y in ys]  # (No, rows+1)
    Bt = [x.T for x in xs]
    if split:
        terms = [(At[0], Bt[0]), (At[0], Bt[1]), (At[1], Bt[0])]
        if mut == "no_head_tail":
            terms = [terms[0], terms[2]]
    else:
        terms = [(At[0], Bt[0])]
    parts, _ = emu_sum(terms, bounds, order)
    ones = np.ones((1, n_rows), np.float32)
    bterms = [(a, ones) for a in (At if mut != "bias_heads_only" else At[:1])]
    bparts, _ = emu_sum(bterms, bounds, order)
    if mut == "slice_twice":
        z = max(i for i, (a, b) in enumerate(bounds) if b > a)
        parts, bparts = parts + [parts[z]], bparts + [bparts[z]]
    if mut == "stale_slice":
        z = max(i for i, (a, b) in enumerate(bounds) if b > a)
        parts[z], bparts[z] = stale[0][z], stale[1][z]
    rnd = _round_near if order == 0 else _round_down
    seq = lambda ps: ps if order == 0 else ps[::-1]
    dW, db = np.zeros_like(parts[0]), np.zeros_like(bparts[0])
    for p in seq(parts):
        dW = rnd(dW.astype(np.float64) + p)
    for p in seq(bparts):
        db = rnd(db.astype(np.float64) + p)
    sc = 1.0 if mut == "no_out_scale" else float(out_scale)
    dW, db = rnd(dW.astype(np.float64) * sc), rnd(db.astype(np.float64) * sc)[:, 0]
    if perm is not None:
        rs, cs = rows_st, cols_st
        if mut == "perm_wrong_axis":
            rs, cs = cs, rs
        if mut == "perm_missing":
            rs = cs = False
        dW, db = scatter_perm(dW, db, perm, rs, cs)
    return dW, db, (parts, bparts)


def emu_data_grad(dy, W, x, order, cls="rounded", out_scale=1.0, mut=None):
    """dx = ((dy W) out_scale) . [x > 0]  in fp32: dy (m,N), W (N,J), x (m,J); "split": dy, W are (head, tail) tuples."""
    if cls == "split":
        (ah, al), (bh, bl) = dy, (W[0].T, W[1].T)
        terms = [(ah, bh), (ah, bl), (al, bh)]
        if mut == "no_head_tail":
            terms = [terms[0], terms[2]]
    else:
        terms = [(np.asarray(dy, np.float32), np.asarray(W, np.float32).T)]
    terms = [(np.asarray(a, np.float32), np.asarray(b, np.float32)) for a, b in terms]
    _, acc = emu_sum(terms, [(0, terms[0][0].shape[1])], order)
    rnd = _round_near if order == 0 else _round_down
    v = rnd(acc.astype(np.float64) * (1.0 if mut == "no_out_scale" else float(out_scale)))
    keep = (x >= 0) if mut == "mask_ge" else (x > 0)
    return np.where(keep, v, np.float32(0))
