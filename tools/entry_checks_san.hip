// Stand-alone host program: the shared entry builders (csrc/pnr_entry.h) and the scatter plan (csrc/pnr_scatter_plan.h) walked
// over the defect table of tests/test_entry_checks_host.py, for a sanitizer build of the HOST code (no GPU, no launch):
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I pixel-nerf_amd/csrc tools/entry_checks_san.hip -o build/entry_checks_san && build/entry_checks_san
//
// Prints one line per group and exits 0 when every defect was refused, every well-formed call accepted, and every plan's
// workspace sections lie in order inside the size the plan reports.
#include <cstdio>
#include <cstring>

#include "pnr_entry.h"
#include "pnr_scatter_plan.h"

static char g_err[512];
int pnr_fail(int code, const char *msg) {
    std::snprintf(g_err, sizeof(g_err), "%s", msg ? msg : "");
    return code;
}
int pnr::device_cus() { return 256; }  // what the library answers without a device (and the MI355X's own count)

using namespace pnr;

static int g_bad = 0;
static void expect(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s (last message: %s)\n", what, g_err); ++g_bad; }
}

static PnrScene scene(int SB, int NS, int Hl, int Wl, int n_focal = 1, int n_c = 1) {
    static float dummy[16];
    PnrScene s = {};
    s.latent_nhwc = dummy; s.poses = dummy; s.focal = dummy; s.c = dummy;
    s.SB = SB; s.NS = NS; s.Hl = Hl; s.Wl = Wl; s.n_focal = n_focal; s.n_c = n_c;
    s.img_w = 64.f; s.img_h = 64.f;
    return s;
}

int main() {
    static float buf[16];
    const SampleLimits all = {GRID_U32, POINTS_TILED, POINTS_F32};
    EvalParams q = {};

    const PnrScene ok = scene(2, 1, 8, 8);
    const PnrScene defects[] = {scene(0, 1, 8, 8), scene(2, 0, 8, 8), scene(2, 1, 1, 8), scene(2, 1, 8, 1), scene(3, 1, 8, 8, 2, 1),
                                scene(3, 1, 8, 8, 1, 2)};
    expect(check_scene(nullptr, "san") == PNR_E_INVALID && std::strstr(g_err, "san: null argument"), "null scene");
    for (const PnrScene &d : defects) {
        expect(check_scene(&d, "san") == PNR_E_INVALID, "check_scene refuses a defective scene");
        expect(ray_samples(q, "san", &d, buf, buf, 2 * d.SB, 2, 8, false, all) == PNR_E_INVALID, "ray_samples refuses a defective scene");
        expect(points(q, "san", &d, buf, buf, 8, all) == PNR_E_INVALID, "points refuses a defective scene");
    }
    expect(check_scene(&ok, "san") == PNR_OK, "well-formed scene");
    std::printf("scene defects walked\n");

    expect(ray_samples(q, "san", &ok, buf, buf, 4, 2, 8, false, all) == PNR_OK && q.P == 32 && q.SB == 2 && q.rays == buf && q.K == 8, "well-formed samples");
    expect(ray_samples(q, "san", &ok, buf, buf, -1, 2, 8, true, all) == PNR_E_INVALID, "R = -1");
    expect(ray_samples(q, "san", &ok, buf, buf, 4, 2, 0, true, all) == PNR_E_INVALID, "K = 0");
    expect(ray_samples(q, "san", &ok, buf, buf, 4, 0, 8, true, all) == PNR_E_INVALID, "rays_per_obj = 0");
    expect(ray_samples(q, "san", &ok, buf, buf, 6, 2, 8, true, all) == PNR_E_INVALID, "R != SB * rays_per_obj");
    expect(ray_samples(q, "san", &ok, (const float *)nullptr, buf, 4, 2, 8, true, all) == PNR_E_INVALID, "null rays");
    expect(ray_samples(q, "san", &ok, buf, nullptr, 4, 2, 8, true, all) == PNR_E_INVALID, "null z");
    expect(ray_samples(q, "san", &ok, buf, buf, 1 << 20, 1 << 19, 1 << 11, true, all) == PNR_E_INVALID, "2^31 points");
    expect(ray_samples(q, "san", &ok, buf, buf, 1 << 20, 1 << 19, 1 << 11, true, {0, 0, 0}) == PNR_OK && q.P == (1LL << 31), "2^31 points, no limit");
    expect(ray_samples(q, "san", &ok, buf, buf, 0, 0 + 1, 8, true, all) == PNR_E_INVALID, "R = 0 with rays_per_obj = 1");
    q = {};
    const PnrScene one = scene(1, 1, 8, 8);
    expect(ray_samples(q, "san", &one, (const float *)nullptr, nullptr, 0, 1, 8, true, all) == PNR_E_INVALID, "R = 0 is not SB * 1");
    expect(points(q, "san", &ok, buf, buf, 8, all) == PNR_OK && q.P == 16 && q.per_obj == 8, "well-formed points");
    expect(points(q, "san", &ok, nullptr, nullptr, 0, all) == PNR_OK && q.P == 0, "no points");
    expect(points(q, "san", &ok, buf, buf, -1, all) == PNR_E_INVALID, "B = -1");
    expect(points(q, "san", &ok, nullptr, buf, 8, all) == PNR_E_INVALID, "null xyz");
    expect(points(q, "san", &ok, buf, buf, 1 << 30, all) == PNR_E_INVALID, "2^31 points (points)");
    const PnrScene over = scene(1, 1, 2897, 2897), fits = scene(1, 1, 2896, 2896);
    expect(ray_samples(q, "san", &over, buf, buf, 2, 2, 8, true, all) == PNR_E_INVALID && std::strstr(g_err, "feature grid too large"), "grid of 2897^2 texels");
    expect(ray_samples(q, "san", &fits, buf, buf, 2, 2, 8, true, all) == PNR_OK, "grid of 2896^2 texels");
    set_packed(q, buf);
    expect(q.wstream == (const char *)buf && (const char *)q.bias == (const char *)buf + BIAS_OFFSET_BYTES, "set_packed");
    std::printf("sample defects walked\n");

    // scatter plans: the pinned shapes of tests/test_entry_checks_host.py, and every form's sections in order inside `bytes`
    struct Pin { int Hl, Wl, n, K; size_t bytes; int single; };
    const Pin pins[] = {{16, 16, 24, 10, 24320, 0},     {40, 40, 24, 10, 24320, 0},     {50, 60, 24, 10, 39876, 1},
                        {64, 64, 24, 10, 39876, 1},     {72, 80, 24, 10, 40116, 1},     {16, 16, 600, 20, 580864, 0},
                        {32, 32, 128, 96, 590080, 0},   {150, 200, 64, 24, 182164, 1},  {33, 97, 200, 16, 373380, 1},
                        {300, 400, 8, 8, 29028, 1},     {64, 131104, 24, 10, 0, 0}};
    for (const Pin &pin : pins) {
        const PnrScene s = scene(2, 2, pin.Hl, pin.Wl);
        expect(scatter_sizes_ok(s, 2 * pin.n, pin.n, pin.K), "scatter sizes");
        const ScatterPlan p = scatter_plan(s, 2 * pin.n, pin.n, pin.K);
        expect(p.bytes == pin.bytes && (p.form == SCATTER_TILED) == (pin.single == 1), "scatter plan pin");
        if (p.form == SCATTER_ATOMIC) continue;
        const size_t P = (size_t)2 * pin.n * pin.K;
        bool ordered = p.coords == 0 && p.segs == (size_t)s.NS * P * 8 && p.segs < p.nseg && p.nseg + (size_t)p.images * SEG_NSUB * 4 <= p.bytes &&
                       p.sub_len % 64 == 0 && (long long)p.sub_len * SEG_NSUB >= (long long)pin.n * pin.K;
        if (p.form == SCATTER_SLAB)
            ordered = ordered && (p.cs == 16 || p.cs == 8 || p.cs == 4) && (p.psplit == 1 || p.psplit == 2) &&
                      (size_t)pin.Hl * pin.Wl * p.row * 8 <= (size_t)SLAB_MAX_BYTES - 128;
        else
            ordered = ordered && p.tile_cnt % 16 == 0 && p.tile_cnt >= p.nseg + (size_t)p.images * SEG_NSUB * 4 && p.tile_cnt < p.tile_off &&
                      p.tile_off < p.cursor && p.cursor < p.entries && p.entries + 16 * (size_t)s.NS * P == p.bytes && p.tiles.ntiles <= 8192;
        expect(ordered, "scatter plan sections");
    }
    expect(!scatter_sizes_ok(ok, 0, 1, 8) && !scatter_sizes_ok(ok, 4, 2, 0) && !scatter_sizes_ok(ok, 6, 2, 8), "scatter sizes refused");
    std::printf("scatter plans walked\n");
    std::printf(g_bad ? "%d FAILED\n" : "all refused / accepted as expected\n", g_bad);
    return g_bad ? 1 : 0;
}
