// pnr_entry.h -- the host prologue of every entry that takes a PnrScene plus ray samples or points, written once: the scene
// check, the size / null / R == SB * rays_per_obj checks, the index limits of the entry's kernels, and the EvalParams the
// kernels take.  Host code only; an entry adds its own checks (dump structs, PnrSplitAux, stream scale, workspace) around it.
#pragma once
#include <cstdio>

#include "pnr_device.h"

namespace pnr {

// PNR_E_INVALID with "<exported name of the entry>: <what>"
inline int entry_fail(const char *entry, const char *what) {
    char msg[256];
    std::snprintf(msg, sizeof(msg), "%s: %s", entry, what);
    return pnr_fail(PNR_E_INVALID, msg);
}

// what is wrong with a scene (nullptr: nothing); the size-returning entries answer 0 on a defect, the others check_scene()
inline const char *scene_defect(const PnrScene *s) {
    if (!s) return "null argument (scene)";
    if (s->SB <= 0 || s->NS <= 0 || s->Hl < 2 || s->Wl < 2) return "bad scene shape (SB > 0, NS > 0, Hl >= 2, Wl >= 2)";
    if (!(s->n_focal == 1 || s->n_focal == s->SB) || !(s->n_c == 1 || s->n_c == s->SB)) return "focal / c must have 1 or SB rows";
    return nullptr;
}
inline int check_scene(const PnrScene *s, const char *entry) {
    const char *d = scene_defect(s);
    return d ? entry_fail(entry, d) : PNR_OK;
}

// elements of the feature grid = of one folded table
inline long long grid_elems(const PnrScene &s) { return (long long)s.SB * s.NS * s.Hl * s.Wl * C_LAT; }

// The index limits an entry's kernels set (0: none), passed by the entry:
struct SampleLimits {
    long long grid;    // elements of the feature grid
    long long points;  // P = R * K (or SB * B)
    long long rows;    // P * NS
};
constexpr long long GRID_U32 = 0xffffffffLL;     // project_point forms texel offsets as 32-bit element indices into the grid / a table
constexpr long long POINTS_TILED = 0x7fffff80LL; // fused kernels: int tile * MT + row, the last tile rounded up to MT = 64 or 96 points
constexpr long long POINTS_F32 = 0x7fffffc0LL;   // unfused fp32 chain: int row index, a launch rounded up to 64 rows
constexpr long long INDEX_I32 = 0x7fffffffLL;    // a point (or view * P + point) index held in an int
constexpr SampleLimits EVAL_LIMITS = {GRID_U32, POINTS_TILED, 0};  // eval_kernel, eval_split_kernel

inline int check_limits(const PnrScene &s, long long P, const SampleLimits &lim, const char *entry) {
    if (lim.points && P > lim.points) return entry_fail(entry, "too many points (P must stay below 2^31)");
    if (lim.rows && P * s.NS > lim.rows) return entry_fail(entry, "too many points (P * NS must stay below 2^31)");
    if (lim.grid && grid_elems(s) > lim.grid)
        return entry_fail(entry, "feature grid too large (SB*NS*Hl*Wl*512 must stay below 2^32 elements)");
    return PNR_OK;
}

// the scene's fields of a launch, the multi-view scratch (PnrScene.mv_workspace) included
inline void scene_params(EvalParams &q, const PnrScene &s) {
    q.latent = s.latent_nhwc; q.poses = s.poses; q.focal = s.focal; q.c = s.c;
    q.SB = s.SB; q.NS = s.NS; q.Hl = s.Hl; q.Wl = s.Wl; q.n_focal = s.n_focal; q.n_c = s.n_c;
    q.img_w = s.img_w; q.img_h = s.img_h;
    q.mv_ws = (float *)s.mv_workspace;
}

inline RaySrc explicit_rays(const float *rays) {
    RaySrc s = {};
    s.rays = rays;
    return s;
}

// (ray, z) samples of a checked scene: rays from `src` (explicit array or camera), z (R,K).  PNR_OK: q holds the scene and
// the samples (q.P == 0 when R == 0 -- allowed only with allow_empty: inference entries then return PNR_OK, training and
// backward entries refuse an empty pass).
inline int ray_samples(EvalParams &q, const char *entry, const PnrScene *s, const RaySrc &src, const float *z, int R, int rays_per_obj,
                       int K, bool allow_empty, const SampleLimits &lim) {
    if (int rc = check_scene(s, entry)) return rc;
    if (R < (allow_empty ? 0 : 1) || K <= 0 || rays_per_obj <= 0) return entry_fail(entry, "bad sizes (R, K, rays_per_obj)");
    if ((long long)rays_per_obj * s->SB != R) return entry_fail(entry, "R != SB * rays_per_obj");
    if (R > 0 && ((!src.rays && !src.poses) || !z)) return entry_fail(entry, "null rays/z");
    const long long P = (long long)R * K;
    if (int rc = check_limits(*s, P, lim, entry)) return rc;
    scene_params(q, *s);
    q.rays = src.rays; q.cam = src; q.cam.rays = nullptr;
    q.z = z; q.K = K; q.per_obj = rays_per_obj; q.P = P;
    return PNR_OK;
}
inline int ray_samples(EvalParams &q, const char *entry, const PnrScene *s, const float *rays, const float *z, int R, int rays_per_obj,
                       int K, bool allow_empty, const SampleLimits &lim) {
    return ray_samples(q, entry, s, explicit_rays(rays), z, R, rays_per_obj, K, allow_empty, lim);
}

// its twin for explicit points: xyz, viewdirs (SB,B,3); B == 0 gives q.P == 0
inline int points(EvalParams &q, const char *entry, const PnrScene *s, const float *xyz, const float *viewdirs, int B,
                  const SampleLimits &lim) {
    if (int rc = check_scene(s, entry)) return rc;
    if (B < 0) return entry_fail(entry, "bad sizes (B)");
    if (B > 0 && (!xyz || !viewdirs)) return entry_fail(entry, "null xyz/viewdirs");
    const long long P = (long long)s->SB * B;
    if (int rc = check_limits(*s, P, lim, entry)) return rc;
    scene_params(q, *s);
    q.xyz = xyz; q.viewdirs = viewdirs; q.K = 1; q.per_obj = B > 0 ? B : 1; q.P = P;
    return PNR_OK;
}

// weight stream, biases and lin_out bias of a packed blob (pnr_pack_mlp*, head blob of a split stream)
inline void set_packed(EvalParams &q, const void *packed) {
    q.wstream = (const char *)packed;
    q.bias = (const float *)((const char *)packed + BIAS_OFFSET_BYTES);
    q.bout = (const float *)((const char *)packed + BOUT_OFFSET_BYTES);
}

}  // namespace pnr
