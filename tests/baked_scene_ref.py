"""numpy restatement of the scene march (include/pixelnerf_hip.h, "Scenes of several baked volumes"), and the inputs the host and
the GPU tests of it share.  Like baked_ref.render_ref it walks the rays, the samples of a ray and the objects at a sample one after
the other in `dtype`: fp64 is the yardstick, fp32 what a correct fp32 implementation of the same formulas differs from it by.

An object is a dict: "stored" (nx,ny,nz,4) with "degree" None, or (nx,ny,nz,B,4) with "degree" 0, 1, 2; "c1", "c2" its box in its own
frame; "pose" (3,4) or (4,4) object-to-world; "occupied" None or (nx-1,ny-1,nz-1) bool.  The inputs proper are rounded to fp32 first
and then carried in `dtype`, as in baked_ref."""
import numpy as np

import baked_ref as B
import baked_sh_ref as SH

common_volume, common_rays, SETTINGS, C1, C2, gaps = B.common_volume, B.common_rays, B.SETTINGS, B.C1, B.C2, B.gaps

IDENTITY = np.eye(4, dtype=np.float32)[:3]
RZ = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], np.float32)   # a quarter turn about z: entries 0 and +-1


def pose_of(rot, t):
    return np.concatenate((np.asarray(rot, np.float32), np.asarray(t, np.float32).reshape(3, 1)), axis=1)


POSE_OVERLAP = pose_of(RZ, (0.25, -0.5, 0.125))    # the boxes of A and B overlap
POSE_DISJOINT = pose_of(RZ, (-1.9375, 0.0, 0.0))   # B stands beside A: 6 of the 37 rays meet it


def obj(stored, pose=IDENTITY, c1=C1, c2=C2, degree=None, occupied=None):
    return {"stored": np.asarray(stored, np.float32), "degree": degree, "c1": c1, "c2": c2, "pose": np.asarray(pose, np.float32)[:3],
            "occupied": occupied}


def object_rays(rays, pose, dtype=np.float32):
    """the world rays (R,8) in the frame of an object: q = o - t, then (q_x R_xa + q_y R_ya) + q_z R_za per axis a, and the same for
    d; every operation rounded on its own in `dtype`; near and far are shared"""
    rays = np.asarray(rays, np.float32).astype(dtype)
    pose = np.asarray(pose, np.float32).astype(dtype)
    rot, t = pose[:3, :3], pose[:3, 3]
    out = rays.copy()
    q = rays[:, 0:3] - t[None, :]
    d = rays[:, 3:6]
    for a in range(3):
        out[:, a] = (q[:, 0] * rot[0, a] + q[:, 1] * rot[1, a]) + q[:, 2] * rot[2, a]
        out[:, 3 + a] = (d[:, 0] * rot[0, a] + d[:, 1] * rot[1, a]) + d[:, 2] * rot[2, a]
    return out


def _value(ob, o, d, t, Y, dtype):
    """the (r,g,b,sigma) of one object at depth t of the ray (o, d) in its frame, or None where it contributes nothing: the
    per-sample part of baked_ref.render_ref / baked_sh_ref.render_ref"""
    dt = np.dtype(dtype).type
    zero, one = dt(0.0), dt(1.0)
    p = o + t * d
    if not (np.all(p >= ob["c1"]) and np.all(p <= ob["c2"])):
        return None
    u = (p - ob["c1"]) / ob["h"]
    cell = np.minimum(np.maximum(np.floor(u), zero), ob["top"])
    f = np.minimum(np.maximum(u - cell, zero), one)
    ix, iy, iz = (int(c) for c in cell)
    if ob["occupied"] is not None and not ob["occupied"][ix, iy, iz]:
        return None
    v = ob["stored"][ix:ix + 2, iy:iy + 2, iz:iz + 2]
    if ob["degree"] is not None:
        v = SH.corner_value(v, Y, dtype)   # clamped per corner, before the blend
    vz = v[:, :, 0] + f[2] * (v[:, :, 1] - v[:, :, 0])   # along z, then y, then x
    vy = vz[:, 0] + f[1] * (vz[:, 1] - vz[:, 0])
    return vy[0] + f[0] * (vy[1] - vy[0])


def render_ref(rays, objects, step, white_bkgd=False, terminate=0.0, dtype=np.float64):
    """rays (R,8) in the world frame, objects a list of obj(...) -> rgb (R,3), depth (R,), alpha (R,) in `dtype`"""
    dt = np.dtype(dtype).type
    rays = np.asarray(rays, np.float32).astype(dtype)
    step, eps, tiny = dt(np.float32(step)), dt(np.float32(terminate)), dt(1e-10)
    half, one, zero = dt(0.5), dt(1.0), dt(0.0)
    obs = []
    for ob in objects:
        reso = ob["stored"].shape[:3]
        c1, c2 = np.asarray(ob["c1"], np.float32).astype(dtype), np.asarray(ob["c2"], np.float32).astype(dtype)
        obs.append({"stored": ob["stored"].astype(dtype), "degree": ob["degree"], "c1": c1, "c2": c2, "h": B.cell_size(c1, c2, reso, dtype),
                    "top": (np.asarray(reso) - 2).astype(dtype), "occupied": ob["occupied"], "rays": object_rays(rays, ob["pose"], dtype)})
    R = rays.shape[0]
    rgb, depth, alpha = np.zeros((R, 3), dtype), np.zeros((R,), dtype), np.zeros((R,), dtype)
    for r in range(R):
        near, far = rays[r, 6], rays[r, 7]
        n = 0
        if np.isfinite(rays[r]).all() and near < far:   # the WORLD ray decides the samples
            count = np.ceil((far - near) / step)
            if count <= B.MAX_SAMPLES:
                n = int(count)
        Ys = [None if ob["degree"] is None else basis(ob["rays"][r, 3:6], ob["degree"], dtype) for ob in obs]
        T = one
        acc = np.zeros((5,), dtype)  # r, g, b, depth, alpha
        for i in range(n):
            t = near + (dt(i) + half) * step
            vals = []
            for ob, Y in zip(obs, Ys):   # in list order
                v = _value(ob, ob["rays"][r, 0:3], ob["rays"][r, 3:6], t, Y, dtype)
                if v is not None:
                    vals.append(v)
            sigma = zero
            for v in vals:
                sigma = sigma + v[3]
            c = np.zeros((3,), dtype)
            if sigma > 0:
                for v in vals:
                    c = c + (v[3] / sigma) * v[0:3]
            a = one - np.exp(-(step * sigma))
            w = a * T
            acc[0:3] += w * c
            acc[3] += w * t
            acc[4] += w
            T = T * (one - a + tiny)
            if eps > 0 and (i + 1) % 64 == 0 and T <= eps:
                break
        if white_bkgd:
            acc[0:3] = acc[0:3] + one - acc[4]
        rgb[r], depth[r], alpha[r] = acc[0:3], acc[3], acc[4]
    return rgb, depth, alpha


def basis(d, degree, dtype=np.float64):
    """baked_sh_ref.sh_basis for ONE direction carried in `dtype`: that function rounds its argument to fp32 first, and a direction
    rotated in fp64 is not fp32-representable.  The same formulas in the same order (on an fp32 direction: the same bits)."""
    dt = np.dtype(dtype).type
    nb = SH.n_basis(degree)
    d = np.asarray(d, dtype)
    c1, c2, c20, c22 = (dt(np.float32(v)) for v in (np.sqrt(3.0), np.sqrt(15.0), np.sqrt(5.0) / 2.0, np.sqrt(15.0) / 2.0))
    Y = np.zeros((nb,), dtype)
    Y[0] = 1
    with np.errstate(all="ignore"):
        n2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        if np.isfinite(n2) and n2 != 0:
            s = np.sqrt(n2)
            x, y, z = d[0] / s, d[1] / s, d[2] / s
            cols = [dt(1.0), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c20 * (dt(3.0) * (z * z) - dt(1.0)), c2 * (x * z),
                    c22 * (x * x - y * y)]
            Y[:] = cols[:nb]
    return Y


def whiten(out):
    """the white-background outputs from the black-background ones: (rgb + 1) - alpha at the end of the walk, the same operations"""
    rgb, depth, alpha = out
    one = rgb.dtype.type(1.0)
    return rgb + one - alpha[:, None], depth, alpha


# ---------------------------------------------------------------- the inputs of tests/test_hip_baked_scene.py (checked on the host too)
SMALL_RESO, SMALL_C1, SMALL_C2 = (5, 6, 4), (-0.5, -0.6, -0.35), (0.45, 0.5, 0.4)   # the second object of the three-object case


def small_volume(seed=5, degree=None):
    """(5,6,4,4) or (5,6,4,B,4): rgb in [0,1], sigma in [0,30] on the inner points and exactly 0 on the outermost layer of every face
    (fp32 and fp64 may disagree on whether a sample near a face is inside); coefficients k >= 1 as baked_sh_ref.common_coef's"""
    rs = np.random.RandomState(seed)
    vol = np.empty(SMALL_RESO + (4,), np.float32)
    vol[..., :3] = rs.uniform(0.0, 1.0, SMALL_RESO + (3,))
    keep = np.zeros(SMALL_RESO, bool)
    keep[1:-1, 1:-1, 1:-1] = True
    vol[..., 3] = np.where(keep, rs.uniform(0.0, 30.0, SMALL_RESO).astype(np.float32), 0.0)
    if degree is None:
        return vol
    coef = np.empty(SMALL_RESO + (SH.n_basis(degree), 4), np.float32)
    coef[..., 0, :] = vol
    coef[..., 1:, :3] = rs.uniform(-0.25, 0.25, SMALL_RESO + (SH.n_basis(degree) - 1, 3))
    sig = rs.uniform(-4.0, 4.0, SMALL_RESO + (SH.n_basis(degree) - 1,)).astype(np.float32)
    coef[..., 1:, 3] = np.where(vol[..., 3][..., None] > 0, sig, np.float32(0.0))
    return coef


def common_coef_b(degree=2):
    """object B of a coefficient scene: baked_sh_ref.common_coef with the DC part of common_volume(seed=99) and other coefficients"""
    coef = SH.common_coef(degree, seed=424242).copy()
    dc = common_volume(seed=99)
    coef[..., 0, :] = dc
    coef[..., 1:, 3] = np.where(dc[..., 3][..., None] > 0, coef[..., 1:, 3], np.float32(0.0))
    return coef


def stored_pair(degree):
    """objects A and B in the shared box: RGBA (degree None) or coefficient volumes"""
    if degree is None:
        return common_volume(), common_volume(seed=99)
    return SH.common_coef(degree), common_coef_b(degree)


def cases(degree):
    """the scenes of the parity test: name -> list of obj(...)"""
    a, b = stored_pair(degree)
    third = pose_of(np.eye(3), (0.0, 0.3, -0.9))
    return {
        "overlap": [obj(a, degree=degree), obj(b, POSE_OVERLAP, degree=degree)],
        "disjoint": [obj(a, degree=degree), obj(b, POSE_DISJOINT, degree=degree)],
        "three": [obj(a, degree=degree), obj(small_volume(degree=degree), pose_of(RZ, (0.9, 0.2, 0.1)), SMALL_C1, SMALL_C2, degree=degree),
                  obj(b, third, degree=degree)],
    }
