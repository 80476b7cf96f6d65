"""
Host tests (no GPU) of tests/gemm_ref.py, the fp64 reference and derived bounds tests/test_hip_gemm_sweep.py holds the GEMMs outside
the fused chains to.

  * an fp32 emulation of each arithmetic class (exact products + fp32 accumulation, rounded products, three-term split) passes
    every bound on every family in two summation orders (one of them rounding every sum toward -inf, as the f16 matrix instruction
    does); on the `exact` family both orders equal the reference BIT FOR BIT -- what licenses the zero-tolerance claim of the sweep;
  * every mutation of the emulation is caught: by any difference on `exact`, by the derived bound on `ranged`.  The miss ratios
    (worst error / bound) measured here are the table in profiles/gemm_sweep_notes.md; the asserted floors are those figures
    rounded down, the only condition set in advance being > 1.
"""
import numpy as np
import pytest

import gemm_ref as G

NO, NK = 24, 24          # output tile of the emulation (the permutation needs a square one)
ROWS, NSPLIT = 70, 3     # slices (0,32) (32,64) (64,70): full slabs and a ragged tail
PERM = G.host_perm(NO)
SCALE = 0.25


def with_guard(v, seed):
    """one more (guard) row of ordinary values behind the rows that count: what a read past the end would pick up"""
    g = np.random.default_rng(77 + seed).integers(1, 4, size=(1, v.shape[1])).astype(np.float32)
    return np.concatenate([v, g], 0)


def operands(cls, family, rows, seed=0):
    """-> (dY, X) fp32 sources (rows + 1, N): the values of the arithmetic class's operand format"""
    if family == "exact":
        if cls == "split":
            dY, X = G.exact_split(rows, NO, rows, seed), G.exact_split(rows, NK, rows, seed + 1)
        else:
            dY, X = G.exact_ints(rows, NO, rows, seed), G.exact_ints(rows, NK, rows, seed + 1)
    elif family == "ranged":
        dY, X = G.ranged(rows, NO, seed, zero_cols=(3,)), G.ranged(rows, NK, seed + 1, zero_cols=(5, 11))
    else:
        dY, X = G.cancelling(rows, NO, seed, flip=False), G.cancelling(rows, NK, seed + 1)
    if cls == "exact":  # 16-bit operands
        dY, X = dY.astype(np.float16).astype(np.float32), X.astype(np.float16).astype(np.float32)
    return with_guard(dY, seed), with_guard(X, seed + 1)


def as_class(cls, v):
    return G.f16_split(v) if cls == "split" else v


def reference(cls, dY, X, rows, nsplit, relu_x=False, rows_st=False, cols_st=False):
    """-> ((dW value, bound), (db value, bound)) from the operand values the emulation is given"""
    terms = 3 if cls == "split" else 1
    if cls == "split":
        (yh, yl), (xh, xl) = G.f16_split(dY[:rows]), G.f16_split(np.maximum(X[:rows], 0) if relu_x else X[:rows])
        ref = G.product_split(yh.T, yl.T, xh.T, xl.T)
        bref = G.product(yh.T.astype(np.float64) + yl.T.astype(np.float64), np.ones((1, rows)))
    else:
        ref = G.product(dY[:rows].T, (np.maximum(X[:rows], 0) if relu_x else X[:rows]).T)
        bref = G.product(dY[:rows].T, np.ones((1, rows)))
    W = G.finish(ref, rows, nsplit, terms=terms, rounded=cls == "rounded", out_scale=SCALE)
    b = G.finish(bref, rows, nsplit, terms=2 if cls == "split" else 1, out_scale=SCALE)
    vW, vb = G.scatter_perm(W[0], b[0][:, 0], PERM, rows_st, cols_st)
    bW, bb = G.scatter_perm(W[1], b[1][:, 0], PERM, rows_st, cols_st)
    return (vW, bW), (vb, bb)


def emulate(cls, dY, X, rows, nsplit, order, **kw):
    return G.emu_weight_grad(as_class(cls, dY), as_class(cls, X), nsplit, order, cls=cls, out_scale=SCALE, perm=PERM, **kw)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("rows,nsplit", [(1, 2), (33, 1), (ROWS, NSPLIT), (257, 4)])
@pytest.mark.parametrize("cls", ["exact", "rounded", "split"])
def test_emulation_passes_every_bound_and_is_bit_exact_on_the_exact_family(cls, rows, nsplit, order):
    for family in ("exact", "ranged", "cancelling"):
        dY, X = operands(cls, family, rows)
        relu = cls == "rounded"
        (vW, bW), (vb, bb) = reference(cls, dY, X, rows, nsplit, relu_x=relu, rows_st=True, cols_st=False)
        dW, db, _ = emulate(cls, dY, X, rows, nsplit, order, relu_x=relu, rows_st=True, cols_st=False)
        if family == "exact":
            assert np.array_equal(dW.astype(np.float64), vW) and np.array_equal(db.astype(np.float64), vb), (cls, rows, order)
        assert G.worst_ratio(dW, vW, bW) <= 1.0 and G.worst_ratio(db, vb, bb) <= 1.0, (cls, family, rows, order)
        if family == "ranged":  # dead features stay dead
            out_row = np.zeros(NO, bool); out_row[PERM[3]] = True
            assert np.all(dW[out_row] == 0) and db[PERM[3]] == 0 and np.all(dW[:, [5, 11]] == 0)


def test_data_gradient_emulation_passes_its_bound():
    m, N, J = 9, 37, 21
    for family in ("exact", "ranged"):
        dy = G.exact_ints(m, N, N, 1) if family == "exact" else G.ranged(m, N, 1)
        W = G.exact_ints(N, J, N, 2) if family == "exact" else G.ranged(N, J, 2, lo=-4, hi=2)
        x = G.exact_ints(m, J, 1, 3)
        value, bound = G.finish(G.product(dy, W.T), N, rounded=True, keep=x > 0)
        for order in (0, 1):
            got = G.emu_data_grad(dy, W, x, order)
            assert G.worst_ratio(got, value, bound) <= 1.0
            if family == "exact":
                assert np.array_equal(got.astype(np.float64), value)


# worst error / bound of each mutation on the `ranged` family, measured here and rounded DOWN (profiles/gemm_sweep_notes.md has the
# unrounded figures); inf: the mutation puts a non-zero where the bound is exactly zero
MEASURED = {
    "drop_tail_slab": 5e4, "row_beyond": 1e36, "slice_twice": 5e4, "stale_slice": 6e12, "perm_wrong_axis": 5e35, "perm_missing": 1e9,
    "no_out_scale": 3e5, "bias_heads_only": 4.9, "no_head_tail": 9.7, "bf16_operand": 180, "no_relu": 2e6, "mask_ge": np.inf,
}

WG_MUTATIONS = [  # (mutation, arithmetic class, emulate keywords)
    ("drop_tail_slab", "exact", {}),
    ("row_beyond", "exact", {}),
    ("slice_twice", "exact", {}),
    ("stale_slice", "exact", {}),
    ("perm_wrong_axis", "exact", {}),
    ("perm_missing", "exact", {}),
    ("no_out_scale", "exact", {}),
    ("bias_heads_only", "split", {}),
    ("no_head_tail", "split", {}),
    ("bf16_operand", "split", {}),
    ("no_relu", "rounded", {"relu_x": True}),
]


def mutation_ratios(name, cls, kw, family):
    """-> (differs anywhere, worst error / bound over dW and db) of one mutated emulation, both orders"""
    dY, X = operands(cls, family, ROWS)
    relu = bool(kw.get("relu_x"))
    (vW, bW), (vb, bb) = reference(cls, dY, X, ROWS, NSPLIT, relu_x=relu, rows_st=True, cols_st=False)
    differs, worst = True, np.inf
    for order in (0, 1):
        stale = None
        if name == "stale_slice":  # the partial sums an earlier call with other operands left behind
            oY, oX = operands(cls, family, ROWS, seed=40)
            stale = emulate(cls, oY, oX, ROWS, NSPLIT, order, rows_st=True, cols_st=False)[2]
        mX = G.trunc_bf16(X) if name == "bf16_operand" else X
        dW, db, _ = emulate(cls, dY, mX, ROWS, NSPLIT, order, rows_st=True, cols_st=False, mut=name, stale=stale, **kw)
        differs &= not (np.array_equal(dW.astype(np.float64), vW) and np.array_equal(db.astype(np.float64), vb))
        worst = min(worst, max(G.worst_ratio(dW, vW, bW), G.worst_ratio(db, vb, bb)))
    return differs, worst


def mask_ratios(family):
    m, N, J = 9, 37, 21
    dy = G.exact_ints(m, N, N, 1) if family == "exact" else G.ranged(m, N, 1)
    W = G.exact_ints(N, J, N, 2) if family == "exact" else G.ranged(N, J, 2, lo=-4, hi=2)
    x = G.exact_ints(m, J, 1, 3)  # holds zeros, positives and negatives
    value, bound = G.finish(G.product(dy, W.T), N, rounded=True, keep=x > 0)
    differs, worst = True, np.inf
    for order in (0, 1):
        got = G.emu_data_grad(dy, W, x, order, mut="mask_ge")
        differs &= not np.array_equal(got.astype(np.float64), value)
        worst = min(worst, G.worst_ratio(got, value, bound))
    return differs, worst


def all_mutation_ratios(family):
    out = {name: mutation_ratios(name, cls, kw, family) for name, cls, kw in WG_MUTATIONS}
    out["mask_ge"] = mask_ratios(family)
    return out


@pytest.mark.parametrize("name", [m[0] for m in WG_MUTATIONS] + ["mask_ge"])
def test_every_mutation_is_caught(name):
    if name == "mask_ge":
        ex, rg = mask_ratios("exact"), mask_ratios("ranged")
    else:
        _, cls, kw = next(m for m in WG_MUTATIONS if m[0] == name)
        ex, rg = mutation_ratios(name, cls, kw, "exact"), mutation_ratios(name, cls, kw, "ranged")
    assert ex[0], f"{name}: the exact family does not see it"
    assert rg[1] > 1.0, f"{name}: inside the bound on the ranged family ({rg[1]:.3g})"
    assert rg[1] >= MEASURED[name], f"{name}: miss ratio {rg[1]:.3g} fell below the recorded {MEASURED[name]:.3g}"


def test_families_are_what_the_module_says():
    for n in (1, 33, 257, 1057, 4000):
        for cap in (8, 256):
            a = G.exact_amax(n, cap)
            assert n * a * a < 2 ** 24 and 1 <= a <= cap
        v = G.exact_split(64, 48, n, 3)
        h, l = G.f16_split(v)
        assert np.array_equal(h.astype(np.float64), np.round(v.astype(np.float64)))  # heads are the integers
        assert set(np.unique(l.astype(np.float64) * 2 ** 12)) <= {-1.0, 0.0, 1.0}
        assert np.array_equal(h.astype(np.float64) + l.astype(np.float64), v.astype(np.float64))
        assert np.all(np.abs(G.exact_ints(64, 48, n, 3, cap=256)) <= G.exact_amax(n, 256))
        assert np.array_equal(G.to_bf16(G.exact_ints(64, 48, n, 3, cap=256)), G.exact_ints(64, 48, n, 3, cap=256))
    # position dependent: no two rows and no two columns of a family member agree
    for v in (G.exact_ints(70, 48, 70), G.exact_split(70, 48, 70)):
        assert len({r.tobytes() for r in v}) == 70 and len({c.tobytes() for c in v.T}) == 48
    r = G.ranged(200, 32, 1, zero_cols=(4,))
    assert np.all(r[:, 4] == 0) and 0.35 < (r == 0).mean() < 0.65
    c = G.cancelling(10, 6, 0)
    assert np.allclose(c[1::2], -c[0::2] * (1 + 2.0 ** -9))
    ref = G.product(G.cancelling(64, 8, 0, flip=False).T, G.cancelling(64, 8, 1).T)
    assert np.all(np.abs(ref.value) < 0.01 * ref.S)  # |ref| << S: a bound relative to |ref| would mean nothing here
    # saturation and subnormal tails of the split
    h, l = G.f16_split(np.array([1e6, -1e6, 2.0 ** -16 * 1.3, 0.1], np.float32))
    assert h[0] == 65504 and h[1] == -65504 and abs(float(l[2])) % 2.0 ** -24 == 0 and abs(0.1 - float(h[3]) - float(l[3])) <= 2.0 ** -25


if __name__ == "__main__":  # the mutation table of profiles/gemm_sweep_notes.md
    ex, rg = all_mutation_ratios("exact"), all_mutation_ratios("ranged")
    print("| mutation | exact family: differs | exact family: error / bound | ranged family: error / bound |")
    print("|---|---|---|---|")
    for k in ex:
        print(f"| {k} | {'yes' if ex[k][0] else 'NO'} | {ex[k][1]:.3g} | {rg[k][1]:.3g} |")
