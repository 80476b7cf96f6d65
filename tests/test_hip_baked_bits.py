"""The bytes of the deterministic baked-volume entries are those of the commit tests/golden/baked_bits.npz was recorded from.

The fixture holds SHA-256 digests of the outputs of the forward march, the ray backward, the scene march and its backward (d_rays,
d_local, d_poses) over all 16 kinds (4 degrees x fp32 / fp16 x dense / sparse), and of the total-variation value and gradient,
recorded on an MI355X by tools/make_baked_bits.py from the library of the commit named in the file (`recorded_from_commit`: the
parent of the commit that split csrc/pnr_baked.hip into a file per concern).  The stored-value backward adds with fp32 atomics, is
not reproducible from run to run and is not here: tests/test_hip_baked_backward.py holds it.

A refactor of these kernels must reproduce the digests.  A later DELIBERATE change of their arithmetic re-records the fixture with
tools/make_baked_bits.py and says so in its commit message.

Inputs: the (9,8,7) volume and the 37 rays of tests/baked_ref.py at 40, 64 and 150 samples (inside a chunk, exactly one chunk,
several chunks), one ray of 4500 samples whose last chunks lie in the box (beyond the 64 chunk heads a wave holds: the rebuild path of
the backward walks), terminate 0 or 1e-2 (stops mid-ray), white background on or off.  Scenes: one object at the identity, and three
objects whose boxes overlap."""
import hashlib
import os

import numpy as np
import pytest
import torch

import baked_ref as B
import sparse_baked_ref as SP

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baked_bits.npz")
KINDS = [(degree, half, sparse) for degree in (None, 0, 1, 2) for half in (False, True) for sparse in (False, True)]
# name -> (near, far, step): n = ceil((far - near) / step)
SETTINGS = {"n40": (1.2, 1.2 + 39.5 * 0.1, 0.1), "n64": (1.2, 1.2 + 63.5 * 0.0625, 0.0625), "n150": (1.2, 1.2 + 149.5 * 0.03, 0.03),
            "n4500": (1.2, 1.2 + 4499.5 * 0.0005, 0.0005)}
TERMINATE = (0.0, 1e-2)
TV_CASES = [(degree, sparse) for degree in (None, 1, 2) for sparse in (False, True)]   # B = 1, 4, 9


def kind_name(degree, half, sparse):
    return f"{'rgba' if degree is None else 'sh%d' % degree}_{'f16' if half else 'f32'}_{'sparse' if sparse else 'dense'}"


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def stored_of(degree, seed=31):
    """the common volume (degree None), or a coefficient volume whose DC part it is: the higher coefficients seeded, large enough
    that the clamps of a corner engage for some directions"""
    vol = B.common_volume()
    if degree is None:
        return vol
    nb = (degree + 1) ** 2
    rs = np.random.RandomState(seed + degree)
    coef = np.zeros(B.RESO + (nb, 4), np.float32)
    coef[..., 0, :] = vol
    coef[..., 1:, :3] = rs.uniform(-0.4, 0.4, B.RESO + (nb - 1, 3))
    coef[..., 1:, 3] = rs.uniform(-4.0, 4.0, B.RESO + (nb - 1,)) * (vol[..., 3:4] > 0)
    return coef


def rays_of(setting):
    near, far, _ = SETTINGS[setting]
    if setting != "n4500":
        rays = B.common_rays("n40").copy()           # the 37 rays, with near and far of this setting where a ray is sampled
        sampled, inside = rays[:, 6] < rays[:, 7], rays[:, 6] == 0.0     # (one ray has near >= far; two start inside the box, near = 0)
        rays[sampled, 7] = np.where(inside[sampled], np.float32(far - near), np.float32(far))
        rays[sampled & ~inside, 6] = np.float32(near)
        return rays
    cam, target = np.array((3.0, 0.3, 0.2)), np.array((-0.2, 0.1, 0.05))
    d = (target - cam) / np.linalg.norm(target - cam)
    return np.concatenate((cam, d, [near, far])).astype(np.float32)[None, :]


def upstream(R, seed=9):
    """d_rgb (R,3), d_depth (R,), d_alpha (R,); ray 5 has none (the row of zeros)"""
    rs = np.random.RandomState(seed)
    ups = [rs.uniform(-1.0, 1.0, (R, 3)).astype(np.float32), rs.uniform(-1.0, 1.0, R).astype(np.float32),
           rs.uniform(-1.0, 1.0, R).astype(np.float32)]
    if R > 5:
        for u in ups:
            u[5] = 0.0
    return ups


def _pose(axis, degrees, t):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(degrees)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    rot = np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)
    return np.concatenate((rot, np.asarray(t, np.float64)[:, None]), axis=1).astype(np.float32)


# three boxes that overlap around the origin
POSES = (np.eye(4, dtype=np.float32)[:3], _pose((0.0, 0.0, 1.0), 90.0, (0.25, -0.5, 0.125)), _pose((0.3, -0.5, 0.8), 37.0, (-0.3, 0.2, 0.35)))


class Volume:
    """one kind on the device: what each entry takes"""

    def __init__(self, degree, half, sparse, dev):
        dense = stored_of(degree)
        self.degree, self.half, self.sparse = degree, half, sparse
        self.bits = self.index = self.ids = None
        stored = dense
        if sparse:
            cells = SP.occupied_cells(B.common_volume()[..., 3], 0.0)
            index, ids = SP.sparse_points(cells)
            self.bits = torch.from_numpy(SP.bits_from_cells(cells).copy().view(np.int32)).to(dev)
            self.index, self.ids = torch.from_numpy(index).to(dev), torch.from_numpy(ids).to(dev)
            stored = np.ascontiguousarray(dense.reshape((-1,) + dense.shape[3:])[ids])
        self.stored32 = torch.from_numpy(stored).to(dev)
        self.stored = self.stored32.half() if half else self.stored32

    def forward(self, ops, rays, step, white, term):
        a = dict(white_bkgd=white, terminate=term)
        if self.sparse:
            fn = ops.baked_sparse_half_render if self.half else ops.baked_sparse_render
            return fn(rays, self.stored, self.degree, self.index, self.bits, B.RESO, B.C1, B.C2, step, **a)
        if self.half:
            return ops.baked_half_render(rays, self.stored, self.degree, B.RESO, B.C1, B.C2, step, **a)
        if self.degree is None:
            return ops.baked_render(rays, self.stored, B.RESO, B.C1, B.C2, step, **a)
        return ops.baked_sh_render(rays, self.stored, self.degree, B.RESO, B.C1, B.C2, step, **a)

    def ray_backward(self, ops, rays, step, ups, white, term):
        return ops.baked_ray_backward(rays, self.stored, self.degree, B.RESO, B.C1, B.C2, step, *ups, bits=self.bits, index=self.index,
                                      white_bkgd=white, terminate=term)

    def objects(self, n):
        return [(self.stored, self.degree, B.RESO, B.C1, B.C2, torch.from_numpy(POSES[j]), self.bits, self.index) for j in range(n)]


def combos(setting):
    """(terminate, white) of a setting: the cross"""
    return [(t, w) for t in TERMINATE for w in (False, True)]


def march_digests(ops, dev, kind):
    """{key: digest} of the forward march and the ray backward of one kind, one key per setting"""
    vol, name, out = Volume(*kind, dev), kind_name(*kind), {}
    for setting, (_, _, step) in SETTINGS.items():
        rays = torch.from_numpy(rays_of(setting)).to(dev)
        ups = [torch.from_numpy(u).to(dev) for u in upstream(rays.shape[0])]
        fwd, bwd = [], []
        for term, white in combos(setting):
            fwd += list(vol.forward(ops, rays, step, white, term))
            bwd.append(vol.ray_backward(ops, rays, step, ups, white, term))
        out[f"forward_{name}_{setting}"] = _digest(*fwd)
        out[f"ray_backward_{name}_{setting}"] = _digest(*bwd)
    return out


def scene_digests(ops, dev, kind):
    """{key: digest} of the scene march and its backward of one kind at N = 1 (identity) and N = 3, one key per (N, setting)"""
    vol, name, out = Volume(*kind, dev), kind_name(*kind), {}
    for n in (1, 3):
        objects = vol.objects(n)
        for setting, (_, _, step) in SETTINGS.items():
            rays = torch.from_numpy(rays_of(setting)).to(dev)
            ups = [torch.from_numpy(u).to(dev) for u in upstream(rays.shape[0])]
            fwd, bwd = [], []
            for term, white in combos(setting):
                fwd += list(ops.baked_scene_render(rays, objects, step, white_bkgd=white, terminate=term))
                bwd += list(ops.baked_scene_backward(rays, objects, step, *ups, white_bkgd=white, terminate=term, want_poses=True))
            out[f"scene_forward_{name}_N{n}_{setting}"] = _digest(*fwd)
            out[f"scene_backward_{name}_N{n}_{setting}"] = _digest(*bwd)
    return out


def tv_digests(ops, dev, case):
    """{key: digest} of the total-variation value (fp32, fp64) and gradient of one (degree, layout)"""
    degree, sparse = case
    vol = Volume(degree, False, sparse, dev)
    nb = 1 if degree is None else (degree + 1) ** 2
    weights = [0.25 + 0.125 * (e % 5) for e in range(4 * nb)]
    grad = torch.zeros_like(vol.stored)
    v32, v64 = ops.baked_tv(vol.stored, degree, B.RESO, weights, eps=1e-6, index=vol.index, ids=vol.ids, want_value=True, grad_out=grad)
    return {f"tv_B{nb}_{'sparse' if sparse else 'dense'}": _digest(v32, v64, grad)}


def all_digests(ops, dev):
    out = {}
    for kind in KINDS:
        out.update(march_digests(ops, dev, kind))
        out.update(scene_digests(ops, dev, kind))
    for case in TV_CASES:
        out.update(tv_digests(ops, dev, case))
    return out


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from pixelnerf_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: str(z[k]) for k in z.files}


def _hold(got, golden):
    assert got, "nothing computed"
    missing = [k for k in got if k not in golden]
    assert not missing, f"not in {os.path.basename(GOLDEN)}: {missing}"
    wrong = [k for k, v in got.items() if golden[k] != v]
    assert not wrong, f"bytes differ from commit {golden['recorded_from_commit']}: {wrong}"


def test_inputs_are_the_cases_the_fixture_names():
    """40, 64, 150 and 4500 samples; 37 rays and one; the long ray's box samples reach beyond chunk 63"""
    for setting, n in (("n40", 40), ("n64", 64), ("n150", 150), ("n4500", 4500)):
        near, far, step = (np.float32(x) for x in SETTINGS[setting])
        assert int(np.ceil((far - near) / step)) == n, setting
        assert rays_of(setting).shape == ((1, 8) if n == 4500 else (37, 8))
    ray, (near, _, step) = rays_of("n4500")[0].astype(np.float64), SETTINGS["n4500"]
    t = near + (np.arange(4096, 4500) + 0.5) * step
    p = ray[None, :3] + t[:, None] * ray[None, 3:6]
    assert ((p > np.array(B.C1) + 0.3) & (p < np.array(B.C2) - 0.3)).all()


@pytest.mark.parametrize("kind", KINDS, ids=[kind_name(*k) for k in KINDS])
def test_march_and_ray_backward_bits(ops, dev, golden, kind):
    _hold(march_digests(ops, dev, kind), golden)


@pytest.mark.parametrize("kind", KINDS, ids=[kind_name(*k) for k in KINDS])
def test_scene_march_and_backward_bits(ops, dev, golden, kind):
    _hold(scene_digests(ops, dev, kind), golden)


@pytest.mark.parametrize("case", TV_CASES, ids=[f"B{1 if d is None else (d + 1) ** 2}_{'sparse' if s else 'dense'}" for d, s in TV_CASES])
def test_tv_bits(ops, dev, golden, case):
    _hold(tv_digests(ops, dev, case), golden)
