// pnr_occgrid.h -- the geometry of a grid of an encoded object (the points of pnr_gen_grid_points, cells of the TRUE spacing) and
// its host checks, shared by the occupancy entries (pnr_occupancy.hip) and the baked-volume ray march (pnr_baked.hip): both assign
// a point to a cell with the same h, so a cell's occupancy bit and its eight corners of a volume are the same cell by construction.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "pnr_common.h"

namespace pnr {

struct OccGrid {
    float c1[3], c2[3], h[3];  // h = (c2 - c1) / (n - 1): util.gen_grid's spacing (util.py:93-110)
    int n[3];                  // grid POINTS per axis; cells: n - 1
};

__device__ __forceinline__ bool occ_finite(float f) { return fabsf(f) <= 3.402823466e+38f; }

inline const char *occ_bad_dims(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return "every axis needs at least 2 grid points";
    if ((long long)(nx - 1) * (ny - 1) * (nz - 1) >= (1LL << 31)) return "the grid must have fewer than 2^31 cells";
    return nullptr;
}

inline int occ_fail(const char *entry, const char *why) {
    char msg[200];
    std::snprintf(msg, sizeof msg, "%s: %s", entry, why);
    return pnr_fail(PNR_E_INVALID, msg);  // (copies the text)
}

// the grid of the clip, the mark and the march entries: c1 / c2 checked, h = (c2 - c1) / (n - 1) rounded once from fp64; nullptr when it is usable
inline const char *occ_grid(int nx, int ny, int nz, const float *c1, const float *c2, OccGrid &g) {
    if (!c1 || !c2) return "c1 / c2 is null (host arrays of 3 floats)";
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(c1[a]) || !std::isfinite(c2[a]) || !(c1[a] < c2[a])) return "c1 / c2 must be finite with c1 < c2 on every axis";
        g.c1[a] = c1[a];
        g.c2[a] = c2[a];
        g.n[a] = n[a];
        g.h[a] = (float)(((double)c2[a] - (double)c1[a]) / (double)(n[a] - 1));
        if (!(g.h[a] > 0.f) || !std::isfinite(g.h[a])) return "the cell size (c2 - c1) / (n - 1) is not a positive fp32 number";
    }
    return nullptr;
}

inline bool occ_misaligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

}  // namespace pnr
