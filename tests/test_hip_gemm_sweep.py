"""
GPU tests (-m gpu): every GEMM outside the fused chains against the fp64 reference and the DERIVED per-element bounds of
tests/gemm_ref.py (derivation and families there; tests/test_gemm_ref_host.py proves them on the CPU; figures in
profiles/gemm_sweep_notes.md).

    ops.weight_grad_batched / ops.weight_grad   dw_kernel<F16|BF16>, dw_split_wide_kernel, dw_reduce_kernel
    ops.lin_out_grad                            lin_out_grad_kernel, lin_out_reduce_kernel
    ops.linear / ops.linear_backward            linear_f32_kernel (both orientations), wgrad_f32_kernel, wgrad_reduce_f32_kernel,
                                                gemm3_kernel<A_KC,B_KC,STAGES> (all three instantiations)

In every case: each operand is a contiguous row range inside a larger NaN-filled buffer (guard rows in front and behind; for a
(2, rows, cols) split operand in front of the heads and behind the tails), so a read past either end poisons the result; after a
warm-up call the cached workspaces of ops._wg_workspace are filled with NaN, so a partial sum that is not written shows; two calls
give identical bits; on the `exact` family the result equals the reference bit for bit, on `ranged` / `cancelling` every element
is inside its bound and every dead feature is exactly 0.0.  Where the C entry is called directly the outputs start NaN-filled with
guards behind them.

PNR_GEMM_SWEEP_REPORT=<path>: the worst error / bound per kernel form is also written there as JSON (it is always printed).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import gemm_ref as G

pytestmark = pytest.mark.gpu

D = 512
RATIOS, WORST = {}, {}  # per kernel form: worst error / bound seen, and the case it was seen in


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst error / derived bound per kernel form:")
    for k in sorted(RATIOS):
        print(f"  {k:42s} {RATIOS[k]:<10.4g} {WORST.get(k, '')}")
    path = os.environ.get("PNR_GEMM_SWEEP_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({k: [RATIOS[k], WORST.get(k, "")] for k in RATIOS}, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------------ plumbing
def place(v, dtype, dev, off=0):
    """numpy (..., cols) -> the same values as a contiguous device tensor INSIDE a NaN-filled buffer: two guard rows in front (rounded
    to 8 elements, so the 16-byte alignment of the operand survives) plus `off` elements (a view at a 4-byte offset), two behind."""
    t = torch.from_numpy(np.ascontiguousarray(v)).to(dtype)
    cols = t.shape[-1]
    front = -(-2 * cols // 8) * 8 + off
    buf = torch.full((front + t.numel() + 2 * cols + 8,), float("nan"), dtype=dtype, device=dev)
    view = buf[front:front + t.numel()].view(t.shape)
    view.copy_(t.to(dev))
    assert view.is_contiguous() and bool(torch.isnan(buf[:front]).all()) and bool(torch.isnan(buf[front + t.numel():]).all())
    return view


def poison_workspaces(ops):
    for w in ops._wg_workspace.values():
        w.fill_(255)  # every fp32 word 0xffffffff: NaN


def check(form, what, got, value, bound, exact, fails):
    g = got.detach().cpu().double().numpy()
    assert g.shape == value.shape, (what, g.shape, value.shape)
    if not np.isfinite(g).all():
        fails.append(f"{what}: {int((~np.isfinite(g)).sum())} non-finite elements")
        return
    r = G.worst_ratio(g, value, bound)
    if form not in RATIOS or not r <= RATIOS[form]:
        RATIOS[form], WORST[form] = (r if np.isfinite(r) else 1e300), what
    if exact and not np.array_equal(g, value):
        bad = np.argwhere(g != value)
        fails.append(f"{what}: {len(bad)} elements differ from the exact reference, first at {tuple(bad[0])}: {g[tuple(bad[0])]!r} != {value[tuple(bad[0])]!r}")
    elif not r <= 1.0:
        i = np.unravel_index(np.argmax(np.where(bound > 0, np.abs(g - value) / np.where(bound > 0, bound, 1), np.where(g != value, np.inf, 0))), g.shape)
        fails.append(f"{what}: error / bound = {r:.4g} at {tuple(int(x) for x in i)} (got {g[i]!r}, reference {value[i]!r}, bound {bound[i]:.3g})")


def to_values(v, dt):
    """fp32 family values -> the values a 16-bit operand of dtype dt holds (as float32)"""
    return torch.from_numpy(v).to(dt).float().numpy()


DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f16x3": torch.float16}


def wg_operands(prec, family, rows, x_cols, seed):
    """-> (dY, X): float32 value arrays (16-bit forms) or (head, tail) float16 tuples (f16x3), per family"""
    if family == "exact":
        if prec == "f16x3":
            dY, X = G.exact_split(rows, D, rows, seed), G.exact_split(rows, x_cols, rows, seed + 1)
        else:
            cap = 256 if prec == "bf16" else 8
            dY, X = G.exact_ints(rows, D, rows, seed, cap), G.exact_ints(rows, x_cols, rows, seed + 1, cap)
    elif family == "ranged":
        dY, X = G.ranged(rows, D, seed, zero_cols=(5, 300)), G.ranged(rows, x_cols, seed + 1, zero_cols=(7, 40))
    else:
        eps = 2.0 ** -6 if prec == "bf16" else 2.0 ** -9
        dY, X = G.cancelling(rows, D, seed, flip=False), G.cancelling(rows, x_cols, seed + 1, eps=eps)
    if prec == "f16x3":
        return G.f16_split(dY), G.f16_split(X)
    return to_values(dY, DT[prec]), to_values(X, DT[prec])


def wg_place(prec, op, dev):
    if prec == "f16x3":
        return place(np.stack([op[0], op[1]]), torch.float16, dev)
    return place(op, DT[prec], dev)


def wg_reference(prec, dY, X, nsplit, out_scale, n_scale_ops, rs, cs, perm, ncw):
    """-> (dW value, dW bound, db value, db bound) in feature order"""
    if prec == "f16x3":
        rows = dY[0].shape[0]
        ref = G.product_split(dY[0].T, dY[1].T, X[0].T, X[1].T)
        bref = G.product(dY[0].T.astype(np.float64) + dY[1].T.astype(np.float64), np.ones((1, rows)))
        terms, bterms = 3, 2
    else:
        rows = dY.shape[0]
        ref, bref = G.product(dY.T, X.T), G.product(dY.T, np.ones((1, rows)))
        terms, bterms = 1, 1
    vW, bW = G.finish(ref, rows, nsplit, terms=terms, out_scale=out_scale, n_scale_ops=n_scale_ops)
    vb, bb = G.finish(bref, rows, nsplit, terms=bterms, out_scale=out_scale, n_scale_ops=n_scale_ops)
    vW, vb = G.scatter_perm(vW[:, :ncw], vb[:, 0], perm, rs, cs)
    bW, bb = G.scatter_perm(bW[:, :ncw], bb[:, 0], perm, rs, cs)
    return vW, bW, vb, bb


def lib_nsplit(n_jobs, max_rows):
    from pixelnerf_amd import _lib
    nbytes = _lib.load().pnr_weight_grad_batched_workspace_bytes(n_jobs, max_rows)
    assert nbytes > 0 and nbytes % (n_jobs * (D * D + D) * 4) == 0
    return nbytes // (n_jobs * (D * D + D) * 4)


def storage_perm(dev):
    from pixelnerf_amd import ops
    return ops.storage_perm(dev).cpu().numpy().astype(np.int64)


def run_batch(dev, prec, family, specs, out_scale=1.0, scale_dev=None, single=False):
    """specs: list of (rows, rows_st, cols_st, x_cols, dw_cols).  One ops.weight_grad_batched call (warm-up, poisoned workspaces,
    second call), every job against its reference.  single: also through ops.weight_grad (16-bit forms, 512 columns)."""
    from pixelnerf_amd import _lib, ops
    p = _lib.PRECISIONS[prec]
    perm = storage_perm(dev)
    form = {"f16": "dw_kernel<F16>", "bf16": "dw_kernel<BF16>", "f16x3": "dw_split_wide_kernel"}[prec]
    ops_, jobs = [], []
    for j, (rows, rs, cs, xc, dc) in enumerate(specs):
        dY, X = wg_operands(prec, family, rows, xc, seed=3 * j + rows)
        ops_.append((dY, X))
        jobs.append((wg_place(prec, dY, dev), wg_place(prec, X, dev), rs, cs, xc, dc))
    sd = None if scale_dev is None else place(np.array([scale_dev], np.float32), torch.float32, dev)
    total = float(out_scale) * (1.0 if scale_dev is None else float(np.float32(scale_dev)))
    pow2 = np.log2(abs(total)) % 1 == 0 and np.log2(abs(float(out_scale))) % 1 == 0
    first = ops.weight_grad_batched(jobs, p, out_scale, out_scale_dev=sd)
    poison_workspaces(ops)
    outs = ops.weight_grad_batched(jobs, p, out_scale, out_scale_dev=sd)
    nsplit = lib_nsplit(len(specs), max(s[0] for s in specs))
    fails = []
    for j, ((rows, rs, cs, xc, dc), (dY, X), (dW, db), (dW1, db1)) in enumerate(zip(specs, ops_, outs, first)):
        what = f"{prec} {family} job {j} rows={rows} st=({rs},{cs}) x_cols={xc} nsplit={nsplit}"
        if not (torch.equal(dW, dW1) and torch.equal(db, db1)):
            fails.append(what + ": two calls differ")
        vW, bW, vb, bb = wg_reference(prec, dY, X, nsplit, total, 0 if pow2 else 2, rs, cs, perm, dc)
        check(form + " dW", what + " dW", dW, vW, bW, family == "exact", fails)
        check(form + " db", what + " db", db, vb, bb, family == "exact", fails)
        if family == "ranged" and rows > 8:
            assert (bW == 0).any() and (bb == 0).any()  # the dead features are in the case
        if single and xc == D and prec == "f16x3":  # ops.weight_grad takes 16-bit dumps only: the C entry, outputs and workspace NaN-filled
            from pixelnerf_amd._ops_common import _p, _stream
            lib = _lib.load()
            buf = torch.empty(D * D + 256 + D + 256, dtype=torch.float32, device=dev)
            ws = torch.empty(lib.pnr_weight_grad_workspace_bytes() // 4, dtype=torch.float32, device=dev)
            res = []
            for _ in range(2):
                buf.fill_(float("nan")); ws.fill_(float("nan"))
                with torch.cuda.device(dev):
                    _lib.check(lib.pnr_weight_grad(_p(jobs[j][0]), _p(jobs[j][1]), rows, p, total, int(rs), int(cs), _p(buf),
                                                   ctypes.c_void_p(buf[D * D + 256:].data_ptr()), _p(ws), _stream()), "pnr_weight_grad")
                res.append(buf.cpu())
            v1 = wg_reference(prec, dY, X, lib_nsplit(1, rows), total, 0 if pow2 else 1, rs, cs, perm, dc)
            if not torch.equal(res[0].nan_to_num(nan=-7.0), res[1].nan_to_num(nan=-7.0)):
                fails.append(what + " (single entry): two calls differ")
            check(form + " dW", what + " dW (single entry)", res[1][:D * D].view(D, D), v1[0], v1[1], family == "exact", fails)
            check(form + " db", what + " db (single entry)", res[1][D * D + 256:D * D + 256 + D], v1[2], v1[3], family == "exact", fails)
            if not bool(torch.isnan(res[1][D * D:D * D + 256]).all() and torch.isnan(res[1][D * D + 256 + D:]).all()):
                fails.append(what + " (single entry): a guard behind an output was written")
        if single and xc == D and prec != "f16x3":
            sW, sb = ops.weight_grad(jobs[j][0], jobs[j][1], p, total, rows_st=rs, cols_st=cs)
            poison_workspaces(ops)
            sW2, sb2 = ops.weight_grad(jobs[j][0], jobs[j][1], p, total, rows_st=rs, cols_st=cs)
            ns1 = lib_nsplit(1, rows)
            v1 = wg_reference(prec, dY, X, ns1, total, 0 if pow2 else 1, rs, cs, perm, dc)
            if not (torch.equal(sW, sW2) and torch.equal(sb, sb2)):
                fails.append(what + " (single entry): two calls differ")
            check(form + " dW", what + " dW (single entry)", sW2, v1[0], v1[1], family == "exact", fails)
            check(form + " db", what + " db (single entry)", sb2, v1[2], v1[3], family == "exact", fails)
    assert not fails, "\n".join(fails)


FLAGS = [(False, False), (True, False), (False, True), (True, True)]
ROWS_SMALL = [1, 31, 32, 33, 63, 64, 65]
ROWS_LARGE = [255, 256, 257, 513]


# ------------------------------------------------------------------------------------------------ weight gradients
@pytest.mark.parametrize("family", ["exact", "ranged", "cancelling"])
@pytest.mark.parametrize("prec", ["f16", "bf16", "f16x3"])
@pytest.mark.parametrize("rows_list", [ROWS_SMALL, ROWS_LARGE], ids=["rows1-65", "rows255-513"])
def test_weight_grad_row_sweep(dev, rows_list, prec, family):
    """one job per launch (the slice count follows the row count) and the single-job entry, around every slab boundary"""
    for i, rows in enumerate(rows_list):
        rs, cs = FLAGS[(i + len(prec)) % 4]
        run_batch(dev, prec, family, [(rows, rs, cs, D, D)], out_scale=0.25, single=True)


@pytest.mark.parametrize("family", ["exact", "ranged"])
@pytest.mark.parametrize("prec", ["f16", "bf16", "f16x3"])
def test_weight_grad_slice_boundaries_and_empty_slices(dev, prec, family):
    """rows = nsplit 32 k - 1, + 0, + 1 (k = 1, 2) next to a ~1000-row job that sets the slice count -- taken from the library, not
    from a CU count -- so the short jobs' slices end exactly at, one before and one behind a slab; a 1-row job: all but one slice
    empty"""
    n_jobs, big = 8, 1000
    nsplit = lib_nsplit(n_jobs, big)
    rows = [nsplit * 32 * k + d for k in (1, 2) for d in (-1, 0, 1)] + [1, big]
    specs = [(r, *FLAGS[i % 4], D, D) for i, r in enumerate(rows)]
    assert len(specs) == n_jobs
    run_batch(dev, prec, family, specs, out_scale=2.0)
    run_batch(dev, prec, family, [(1, True, True, D, D), (big + 1, True, False, D, D)])


@pytest.mark.parametrize("prec,family", [("f16", "exact"), ("bf16", "exact"), ("f16x3", "ranged")])
def test_weight_grad_thirty_two_slices(dev, prec, family):
    """the largest slice count (one job of >= 7937 rows): 31 full slices of 256 rows and a ragged last one of 63; the split form's
    exact family ends at 4000 rows (tests/gemm_ref.py), so it runs `ranged` here"""
    assert lib_nsplit(1, 7999) > lib_nsplit(1, 1000)
    run_batch(dev, prec, family, [(7999, True, True, D, D)], out_scale=0.5)


@pytest.mark.parametrize("prec", ["f16", "bf16", "f16x3"])
def test_weight_grad_all_storage_orders_exact(dev, prec):
    run_batch(dev, prec, "exact", [(65, rs, cs, D, D) for rs, cs in FLAGS] + [(65, True, False, 64, 42), (65, False, False, 64, 42)])


@pytest.mark.parametrize("prec", ["f16", "bf16", "f16x3"])
def test_weight_grad_sixteen_jobs(dev, prec):
    specs = [(33 + 7 * j, *FLAGS[j % 4], D, D) for j in range(15)] + [(40, True, False, 64, 42)]
    run_batch(dev, prec, "exact", specs)
    run_batch(dev, prec, "ranged", specs)


@pytest.mark.parametrize("prec", ["f16", "bf16", "f16x3"])
def test_weight_grad_out_scale_host_device_and_both(dev, prec):
    specs = [(97, True, True, D, D), (40, True, False, 64, 42)]
    for host, device in ((0.125, None), (1.0, 0.125), (4.0, 2.0 ** -5)):   # powers of two: the exact family stays exact
        run_batch(dev, prec, "exact", specs, out_scale=host, scale_dev=device)
    for host, device in ((0.3, None), (1.0, 0.3), (1.7, 0.3)):
        run_batch(dev, prec, "ranged", specs, out_scale=host, scale_dev=device)


def mlp_specs(P, NS):
    """the 14 jobs of autograd._mlp_grads: blocks 0-2 per view (NS P rows), blocks 3-4 pooled (P rows), lin_z, lin_in"""
    specs = []
    for b in range(5):
        rows = NS * P if b < 3 else P
        specs += [(rows, True, True, D, D), (rows, True, True, D, D)]
    specs += [(NS * P, True, False, D, D)] * 3
    specs.append((NS * P, True, False, 64, 42))
    return specs


@pytest.mark.parametrize("family", ["exact", "ranged"])
@pytest.mark.parametrize("prec", ["f16", "bf16", "f16x3"])
def test_weight_grad_mlp_wiring_through_the_c_entry(dev, prec, family):
    """pnr_weight_grad_batched called directly with the 14 jobs of one ResnetFC backward: outputs NaN-filled, a guard behind every
    dW (the (512,42) one included) and db; every element comes back finite, every guard untouched"""
    from pixelnerf_amd import _lib, ops
    from pixelnerf_amd._ops_common import _p, _stream
    lib = _lib.load()
    P, NS = 67, 3
    specs = mlp_specs(P, NS)
    n = len(specs)
    perm = storage_perm(dev)
    form = {"f16": "dw_kernel<F16>", "bf16": "dw_kernel<BF16>", "f16x3": "dw_split_wide_kernel"}[prec]
    inv = place(np.array([0.5], np.float32), torch.float32, dev)
    GUARD = 512
    sizes = [(D * dc, D) for (_, _, _, _, dc) in specs]
    out = torch.full((sum(a + b + 2 * GUARD for a, b in sizes),), float("nan"), dtype=torch.float32, device=dev)
    arr = (_lib.PnrWeightGradJob * n)()
    keep, values, spans, o = [], [], [], 0
    for j, (rows, rs, cs, xc, dc) in enumerate(specs):
        dY, X = wg_operands(prec, family, rows, xc, seed=11 * j)
        tY, tX = wg_place(prec, dY, dev), wg_place(prec, X, dev)
        keep.append((tY, tX)); values.append((dY, X))
        w0, b0 = o, o + sizes[j][0] + GUARD
        spans.append((w0, b0))
        o = b0 + D + GUARD
        arr[j].dY, arr[j].X, arr[j].rows = tY.data_ptr(), tX.data_ptr(), rows
        arr[j].rows_storage_order, arr[j].cols_storage_order = int(rs), int(cs)
        arr[j].dW, arr[j].db = out[w0:].data_ptr(), out[b0:].data_ptr()
        arr[j].x_cols, arr[j].dw_cols = xc, dc
    assert o == out.numel()
    max_rows = max(s[0] for s in specs)
    nbytes = lib.pnr_weight_grad_batched_workspace_bytes(n, max_rows)
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=dev)
    nsplit = lib_nsplit(n, max_rows)
    results = []
    for _ in range(2):
        out.fill_(float("nan")); ws.fill_(float("nan"))
        with torch.cuda.device(dev):
            _lib.check(lib.pnr_weight_grad_batched(arr, n, _lib.PRECISIONS[prec], 1.0, _p(inv), _p(ws), _stream()), "pnr_weight_grad_batched")
        results.append(out.clone())
    assert torch.equal(results[0].nan_to_num(nan=-7.0), results[1].nan_to_num(nan=-7.0)), "two calls differ"
    res, fails = results[1].cpu(), []
    written = torch.zeros(out.numel(), dtype=torch.bool)
    for j, ((rows, rs, cs, xc, dc), (dY, X), (w0, b0)) in enumerate(zip(specs, values, spans)):
        written[w0:w0 + D * dc] = True
        written[b0:b0 + D] = True
        what = f"{prec} {family} mlp job {j} rows={rows} st=({rs},{cs}) x_cols={xc}"
        vW, bW, vb, bb = wg_reference(prec, dY, X, nsplit, 0.5, 0, rs, cs, perm, dc)
        check(form + " dW", what + " dW", res[w0:w0 + D * dc].view(D, dc), vW, bW, family == "exact", fails)
        check(form + " db", what + " db", res[b0:b0 + D], vb, bb, family == "exact", fails)
    assert bool(torch.isnan(res[~written]).all()), "a guard behind an output was written"
    assert bool(torch.isfinite(res[written]).all())
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("family", ["exact", "ranged", "cancelling"])
@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_lin_out_grad_sweep(dev, prec, family):
    """lin_out: dW (4,512) = g^T x5 (fp32 x 16-bit, storage -> feature order), db (4) = column sums of g; 256 row slices"""
    from pixelnerf_amd import _lib, ops
    perm = storage_perm(dev)
    fails = []
    for P in (1, 255, 256, 257, 1000):
        if family == "exact":
            g, x5 = G.exact_ints(P, 4, P, 1), G.exact_ints(P, D, P, 2, 256 if prec == "bf16" else 8)
        elif family == "ranged":
            g, x5 = G.ranged(P, 4, 1, zero_cols=(2,)), to_values(np.abs(G.ranged(P, D, 2, zero_cols=(9, 400))), DT[prec])
        else:
            g, x5 = G.cancelling(P, 4, 1), to_values(np.abs(G.cancelling(P, D, 2, flip=False)), DT[prec])
        tg, tx = place(g, torch.float32, dev), place(x5, DT[prec], dev)
        first = ops.lin_out_grad(tg, tx, _lib.PRECISIONS[prec])
        poison_workspaces(ops)
        dW, db = ops.lin_out_grad(tg, tx, _lib.PRECISIONS[prec])
        what = f"lin_out {prec} {family} P={P}"
        if not (torch.equal(dW, first[0]) and torch.equal(db, first[1])):
            fails.append(what + ": two calls differ")
        per = -(-P // 256)
        vW, bW = G.finish(G.product(g.T, x5.T), per, 256, rounded=True)
        vb, bb = G.finish(G.product(g.T, np.ones((1, P))), per, 256)
        vW, _ = G.scatter_perm(vW, None, perm, False, True)
        bW, _ = G.scatter_perm(bW, None, perm, False, True)
        check("lin_out_grad_kernel dW", what + " dW", dW, vW, bW, family == "exact", fails)
        check("lin_out_grad_kernel db", what + " db", db, vb[:, 0], bb[:, 0], family == "exact", fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ generic GEMMs
DIMS = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130]
TRIPLES = [(DIMS[i % 15], DIMS[(4 * i + 1) % 15], DIMS[(7 * i + 2) % 15]) for i in range(36)] + \
          [(1023, 33, 5), (1024, 64, 130), (1025, 3, 63), (1057, 129, 2)]   # 32 slices of the split-K weight gradient, ragged


def lin_operands(prec, family, rows, d_in, d_out, seed):
    n = max(rows, d_in, d_out)
    if family == "exact":
        gen = G.exact_split if prec == "f16x3" else G.exact_ints
        x, W, dy = gen(rows, d_in, n, seed), gen(d_out, d_in, n, seed + 1), gen(rows, d_out, n, seed + 2)
        b = ((np.arange(d_out) * 5 + seed) % 7 - 3).astype(np.float32)
        r = ((np.arange(rows)[:, None] * 3 + np.arange(d_out)[None, :] * 5 + seed) % 5 - 2).astype(np.float32)
    elif family == "ranged":
        x = G.ranged(rows, d_in, seed, zero_cols=(1,) if d_in > 2 else ())
        W = G.ranged(d_out, d_in, seed + 1, lo=-6, hi=2)
        dy = G.ranged(rows, d_out, seed + 2, zero_cols=(0,) if d_out > 2 else ())
        b, r = G.ranged(1, d_out, seed + 3, lo=-3, hi=1)[0], G.ranged(rows, d_out, seed + 4, lo=-3, hi=3)
    else:
        f = np.where(np.arange(rows) % 2 == 1, -(1.0 + 2.0 ** -9), 1.0)[:, None]
        x = (np.repeat(G.cancelling((rows + 1) // 2, d_in, seed, along=1), 2, axis=0)[:rows] * f).astype(np.float32)
        w0 = np.random.default_rng(seed + 1).standard_normal(((d_out + 1) // 2, (d_in + 1) // 2))
        W = np.repeat(np.repeat(w0, 2, 0), 2, 1)[:d_out, :d_in].astype(np.float32)
        dy = np.repeat(G.cancelling((rows + 1) // 2, d_out, seed + 2, along=1), 2, axis=0)[:rows].astype(np.float32)
        b, r = G.ranged(1, d_out, seed + 3, lo=-12, hi=-8)[0], G.ranged(rows, d_out, seed + 4, lo=-12, hi=-8)
    return x, W, b, r, dy


def lin_reference(prec, x, W, b, r, dy, relu, s):
    """-> {name: (value, bound, plain value, contract bound)}; s: the gradient scale the device picked (f16x3)"""
    rows, d_in = x.shape
    d_out = W.shape[0]
    xr = np.maximum(x, 0) if relu else x
    keep = (x > 0) if relu else None
    ones = np.ones((1, rows))
    x64, W64, dy64 = xr.astype(np.float64), W.astype(np.float64), dy.astype(np.float64)
    plain = {"y": x64 @ W64.T + (0 if b is None else b.astype(np.float64)[None, :]) + (0 if r is None else r.astype(np.float64)),
             "dx": (dy64 @ W64) * (1.0 if keep is None else keep), "dw": dy64.T @ x64, "db": dy64.sum(0)}
    out = {}
    if prec == "f32":
        out["y"] = G.finish(G.product(xr, W), d_in, rounded=True, bias=b, yin=r)
        out["dx"] = G.finish(G.product(dy, W.T), d_out, rounded=True, keep=keep)
        out["dw"] = G.finish(G.product(dy.T, xr.T), rows, 32, rounded=True)
        extra = {k: 0.0 for k in plain}
        tol = 2e-6
    else:
        (xh, xl), (wh, wl), (gh, gl) = G.f16_split(xr), G.f16_split(W), G.f16_split(dy, s)
        ry, rx, rw = G.product_split(xh, xl, wh, wl), G.product_split(gh, gl, wh.T, wl.T), G.product_split(gh.T, gl.T, xh.T, xl.T)
        out["y"] = G.finish(ry, d_in, terms=3, bias=b, yin=r)
        out["dx"] = G.finish(rx, d_out, terms=3, out_scale=1.0 / s, keep=keep)
        out["dw"] = G.finish(rw, rows, 32, terms=3, out_scale=1.0 / s)
        gs = dy.astype(np.float64) * s
        extra = {"y": ry.drop + G.split_residual(xr, xh, xl, W, wh, wl),
                 "dx": (rx.drop + G.split_residual(gs, gh, gl, W.T, wh.T, wl.T)) / s * (1.0 if keep is None else keep),
                 "dw": (rw.drop + G.split_residual(gs.T, gh.T, gl.T, xr.T, xh.T, xl.T)) / s, "db": 0.0}
        tol = 2e-5
    vb, bb = G.finish(G.product(dy.T, ones), rows, 32 + 8)
    out["db"] = (vb[:, 0], bb[:, 0])
    return {k: (out[k][0], out[k][1], plain[k], G.contract_bound(plain[k], tol, out[k][1], extra[k])) for k in out}


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("case", range(len(TRIPLES)), ids=[f"{i}-{r}x{i_}x{o}" for i, (r, i_, o) in enumerate(TRIPLES)])
def test_linear_and_its_backward_sweep(dev, case, prec):
    """y, dx, dw, db of ops.linear / ops.linear_backward per element; the options rotate with the case: relu_in, residual, bias,
    operands at a 4-byte offset, and the partial requests (need_dx / need_dw / need_db)"""
    from pixelnerf_amd import ops
    rows, d_in, d_out = TRIPLES[case]
    relu, resid, bias, off = case % 2 == 1, case % 3 == 0, case % 4 != 3, 1 if case % 5 in (1, 3) else 0
    tag = {"f32": ("linear_f32_kernel", "linear_f32_kernel (w_trans)", "wgrad_f32_kernel"),
           "f16x3": ("gemm3_kernel<1,1,1>", "gemm3_kernel<1,0,1>", "gemm3_kernel<0,0,2>")}[prec]
    fails = []
    for family in ("exact", "ranged", "cancelling"):
        x, W, b, r, dy = lin_operands(prec, family, rows, d_in, d_out, seed=case)
        b, r = (b if bias else None), (r if resid else None)
        tx, tW, tdy = place(x, torch.float32, dev, off), place(W, torch.float32, dev, off), place(dy, torch.float32, dev, off)
        tb = None if b is None else place(b, torch.float32, dev, off)
        tr = None if r is None else place(r, torch.float32, dev, off)
        s = float(ops.grad_scale(tdy)[0].cpu()) if prec == "f16x3" else 1.0
        assert s > 0 and np.log2(s) % 1 == 0
        ref = lin_reference(prec, x, W, b, r, dy, relu, s)
        y = ops.linear(tx, tW, tb, relu_in=relu, residual=tr, precision=prec)
        y2 = ops.linear(tx, tW, tb, relu_in=relu, residual=tr, precision=prec)
        dx, dw, db = ops.linear_backward(tdy, tx, tW, relu_in=relu, precision=prec)
        dx2, dw2, db2 = ops.linear_backward(tdy, tx, tW, relu_in=relu, precision=prec)
        what = f"{prec} {family} rows={rows} d_in={d_in} d_out={d_out} relu={relu} residual={resid} bias={bias} offset={off}"
        for a, a2, name in ((y, y2, "y"), (dx, dx2, "dx"), (dw, dw2, "dw"), (db, db2, "db")):
            if not torch.equal(a, a2):
                fails.append(f"{what} {name}: two calls differ")
        for got, name, form in ((y, "y", tag[0]), (dx, "dx", tag[1]), (dw, "dw", tag[2]), (db, "db", tag[2] + " db")):
            v, bnd, plain, cb = ref[name]
            check(form, f"{what} {name}", got, v, bnd, family == "exact", fails)
            g = got.detach().cpu().double().numpy()
            if not np.all(np.abs(g - plain) <= cb):
                fails.append(f"{what} {name}: outside the contract bound, worst {float(np.max(np.abs(g - plain) / np.maximum(cb, 1e-300))):.4g}")
        # partial requests: the same bits, nothing else allocated
        a = ops.linear_backward(tdy, tx, tW, relu_in=relu, need_dx=False, need_db=False, precision=prec)
        c = ops.linear_backward(tdy, tx, tW, relu_in=relu, need_dw=False, need_db=False, precision=prec)
        e = ops.linear_backward(tdy, tx, tW, relu_in=relu, need_dx=False, need_dw=False, need_db=True, precision=prec)
        if not (a[0] is None and a[2] is None and torch.equal(a[1], dw)):
            fails.append(f"{what}: need_dw alone differs")
        if not (c[1] is None and c[2] is None and torch.equal(c[0], dx)):
            fails.append(f"{what}: need_dx alone differs")
        if not (e[0] is None and torch.equal(e[2], db) and torch.equal(e[1], dw)):
            fails.append(f"{what}: need_db alone differs")
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("case", [0, 3, 7, 12, 21, 33, 36, 39], ids=lambda c: f"{c}-{'x'.join(map(str, TRIPLES[c]))}")
def test_linear_through_the_c_entries(dev, case, prec):
    """pnr_linear / pnr_linear_backward called directly: y, dx, dw, db start NaN-filled with a guard behind each, the split-K
    workspace starts NaN-filled (a partial sum that is not written shows); every element comes back finite and inside its bound,
    every guard stays untouched, two calls give the same bits"""
    from pixelnerf_amd import _lib, ops
    from pixelnerf_amd._ops_common import _p, _stream
    lib = _lib.load()
    rows, d_in, d_out = TRIPLES[case]
    relu, resid = case % 2 == 1, case % 3 == 0
    P = _lib.PRECISIONS[prec]
    tag = {"f32": ("linear_f32_kernel", "linear_f32_kernel (w_trans)", "wgrad_f32_kernel"),
           "f16x3": ("gemm3_kernel<1,1,1>", "gemm3_kernel<1,0,1>", "gemm3_kernel<0,0,2>")}[prec]
    GUARD = 256
    sizes = {"y": rows * d_out, "dx": rows * d_in, "dw": d_out * d_in, "db": d_out}
    span, o = {}, 0
    for k, n in sizes.items():
        span[k] = (o, o + n)
        o += n + GUARD
    out = torch.empty(o, dtype=torch.float32, device=dev)
    nbytes = lib.pnr_linear_backward_workspace_bytes(d_in, d_out)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    fails = []
    for family in ("exact", "ranged"):
        x, W, b, r, dy = lin_operands(prec, family, rows, d_in, d_out, seed=100 + case)
        r = r if resid else None
        tx, tW, tdy, tb = (place(v, torch.float32, dev) for v in (x, W, dy, b))
        tr = None if r is None else place(r, torch.float32, dev)
        sc = ops.grad_scale(tdy)
        s = float(sc[0].cpu()) if prec == "f16x3" else 1.0
        ref = lin_reference(prec, x, W, b, r, dy, relu, s)
        results = []
        for _ in range(2):
            out.fill_(float("nan")); ws.fill_(float("nan"))
            ptr = {k: ctypes.c_void_p(out[a:].data_ptr()) for k, (a, _) in span.items()}
            with torch.cuda.device(dev):
                _lib.check(lib.pnr_linear(_p(tx), _p(tW), _p(tb), _p(tr), ptr["y"], rows, d_in, d_out, int(relu), P, _stream()), "pnr_linear")
                _lib.check(lib.pnr_linear_backward(_p(tdy), _p(tx), _p(tW), rows, d_in, d_out, int(relu), ptr["dx"], ptr["dw"], ptr["db"],
                                                   _p(sc), _p(ws), nbytes, P, _stream()), "pnr_linear_backward")
            results.append(out.cpu())
        what = f"C entry {prec} {family} rows={rows} d_in={d_in} d_out={d_out} relu={relu} residual={resid}"
        if not torch.equal(results[0].nan_to_num(nan=-7.0), results[1].nan_to_num(nan=-7.0)):
            fails.append(what + ": two calls differ")
        res, written = results[1], torch.zeros(o, dtype=torch.bool)
        for (k, (a, e)), form, shape in zip(span.items(), (tag[0], tag[1], tag[2], tag[2] + " db"),
                                            ((rows, d_out), (rows, d_in), (d_out, d_in), (d_out,))):
            written[a:e] = True
            check(form, f"{what} {k}", res[a:e].view(shape), ref[k][0], ref[k][1], family == "exact", fails)
        if not bool(torch.isnan(res[~written]).all()):
            fails.append(what + ": a guard behind an output was written")
    assert not fails, "\n".join(fails[:20])
