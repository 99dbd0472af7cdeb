// Launch plan shared by the persistent Winograd forward / dgrad kernels (winograd24.hip: nested F(2,3)xF(4,3);
// winograd44f.hip: F(4x4,3x3)): how a grid of T equal workgroup tiles is finished on 256 CUs, in ONE function
// (wino_launch_plan) that the launchers execute and every host query reads (workspace, fill, GroupNorm fusion, plan).
#pragma once
#include <cstddef>
#include <cstdlib>

namespace {

constexpr int WINO_SLOTS = 256;       // one workgroup per CU
constexpr double WINO_TAIL_G = 4.0;   // cost of the fix-up launch behind a split tail, in chunk-times
constexpr double WINO_TAIL_F = 2.5;   // per-part overhead of a K-split tail part, in chunk-times (see wino_tail_time)

inline int rup(int v, int m) { return (v + m - 1) / m * m; }

// A workgroup = CO output channels x TT output tiles x SLICES Winograd slices, fed CK input channels per chunk; a K-split
// tail part leaves TILE_FLOATS raw outputs per (channel, tile) in the workspace, a fix-up thread finishes FIXUP_FLOATS.
struct WinoNested {                   // winograd24.hip: 2x4 output tiles
    static constexpr int SLICES = 24, CO = 64, CK = 8, TT = 32, TILE_FLOATS = 8, FIXUP_FLOATS = 8, PERSIST = WINO_SLOTS;
    static bool supported(int H, int W, int mode) {
        return H == W && (W == 8 || W == 16 || W == 32 || W == 64) && (mode == 0 || mode == 2);
    }
    // tiles of a launch: groups of 32 output tiles (256 pixels) x 64-channel tiles; an 8x8 map packs four views into one
    static int groups(int S, int H, int W) {
        const int tiles = (H / 2) * (W / 4);
        return tiles >= TT ? S * (tiles / TT) : (S + TT / tiles - 1) / (TT / tiles);
    }
};
struct WinoF44 {                      // winograd44f.hip: 4x4 output tiles (512 pixels per group)
    static constexpr int SLICES = 36, CO = 64, CK = 8, TT = 32, TILE_FLOATS = 16, FIXUP_FLOATS = 4, PERSIST = WINO_SLOTS;
    static bool supported(int H, int W, int mode) { return H == W && (W == 32 || W == 64) && (mode == 0 || mode == 2); }
    static int groups(int S, int H, int W) { return S * ((H / 4) * (W / 4) / TT); }
};

// How a grid of T equal tiles is finished when T is not a multiple of the slot count: the last R = T mod 256
// tiles are split over K into `split` parts each; the parts run in ceil(R*split/256) rounds.  A part of `per` chunks
// costs per + F chunk-times, F = the prologue + epilogue + partial-output store of a workgroup in units of one chunk
// (measured: a tile's epilogue is 23 % of an 8-chunk tile; VF_WINO_TAIL_F overrides, tuning aid).  `split` is the value
// in [1, min(8, nch/4)] with the shortest tail (ties: fewer parts).
inline double wino_tail_overhead() {
    static const double f = getenv("VF_WINO_TAIL_F") ? atof(getenv("VF_WINO_TAIL_F")) : WINO_TAIL_F;
    return f;
}
inline double wino_tail_fixup() {     // the fix-up launch a split costs, in chunk-times (VF_WINO_TAIL_G overrides, tuning aid)
    static const double g = getenv("VF_WINO_TAIL_G") ? atof(getenv("VF_WINO_TAIL_G")) : WINO_TAIL_G;
    return g;
}
inline double wino_tail_time(int R, int sp, int nch, double F) {      // in units of one whole tile
    const int per = (nch + sp - 1) / sp;
    const double fix = (sp > 1 && F > 0.0) ? wino_tail_fixup() : 0.0;
    return ((double)((R * sp + WINO_SLOTS - 1) / WINO_SLOTS) * (per + F) + fix) / (nch + F);
}

inline void wino_tail_plan(int T, int nch, int* nfull, int* split, double F) {
    *nfull = T;
    *split = 1;
    const int R = T % WINO_SLOTS;
    if (R == 0 || T / WINO_SLOTS >= 3) return;          // tail round costs < 1/4 of the launch: leave it
    int best = 1;
    for (int sp = 2; sp <= 8 && sp <= nch / 4; ++sp) {    // at least 4 chunks per part
        const int per = (nch + sp - 1) / sp;              // the kernel gives each part `per` chunks:
        if ((nch + per - 1) / per != sp) continue;        // no part may start beyond the last chunk
        if (wino_tail_time(R, sp, nch, F) < wino_tail_time(R, best, nch, F) - 1e-9) best = sp;
    }
    if (best < 2) return;
    *nfull = T - R;
    *split = best;
}

// One launch of T tiles over nch chunks: `per` chunks per K range of a tail tile (the last may be shorter); the raw
// partials (ws_need floats) are summed by a fix-up launch of fixup_grid workgroups (0: no tail, no fix-up).
struct WinoLaunchPlan {
    int T, nch, nfull, split, per, npers, conv_grid, fixup_grid;
    long ws_need;
    bool all_split() const { return nfull == 0 && split >= 2; }     // every tile a K-split tail tile
};

struct WinoArgs {      // what both conv kernels and their fix-ups take
    const float* x;
    const float* u;       // packed transformed weights
    const float* bias;
    const float* vbias;
    const float* res;
    float* y;
    int S, Cin, Cout, CinP, CoutP;
    // tail splitting (small maps): tiles [0, nfull) are computed whole (by the persistent workgroups); workgroup
    // npers + j*tail_split + p computes the p-th K range of tile nfull + j and leaves a raw partial output in ws
    // (the fix-up kernels)
    int nfull, tail_split;
    float* ws;
    int npers;            // persistent workgroups = min(nfull, PERSIST)
};

constexpr size_t WINO_WS_ANY = ~(size_t)0;     // "whatever the plan wants": the unclamped plan

// The plan of kernel K at this shape with the workspace actually available.  Parts that do not fit, or no workspace:
// the plain grid (every tile whole).  F: the per-part overhead the split search prices (0: pure occupancy).
template <class K>
inline WinoLaunchPlan wino_launch_plan(int S, int Cin, int Cout, int H, int W, bool has_ws, size_t ws_floats,
                                       double F = wino_tail_overhead()) {
    WinoLaunchPlan p;
    p.T = K::groups(S, H, W) * (rup(Cout, K::CO) / K::CO);
    p.nch = rup(Cin, K::CK) / K::CK;
    wino_tail_plan(p.T, p.nch, &p.nfull, &p.split, F);
    constexpr int PART = K::CO * K::TT * K::TILE_FLOATS;            // raw partial output of one tail part
    if ((size_t)(p.T - p.nfull) * p.split * PART > ws_floats || !has_ws) {   // no room: plain grid
        p.nfull = p.T;
        p.split = 1;
    }
    const int nt = p.T - p.nfull;
    p.per = (p.nch + p.split - 1) / p.split;
    p.npers = p.nfull < K::PERSIST ? p.nfull : K::PERSIST;
    p.conv_grid = p.npers + nt * p.split;
    p.fixup_grid = (nt * (PART / K::FIXUP_FLOATS) + 255) / 256;
    p.ws_need = (long)nt * p.split * PART;
    return p;
}

// Expected CU fill (percent) of the launch, and the tile count; hosts use it to choose between the Winograd paths and
// the direct kernel.  (Pure occupancy figure: the tail is priced WITHOUT the per-part overhead that the launch's own
// plan uses, so the hosts' thresholds keep their meaning.)
template <class K>
inline int wino_fill_pct(int S, int Cin, int Cout, int H, int W, int* tiles_out) {
    const WinoLaunchPlan p = wino_launch_plan<K>(S, Cin, Cout, H, W, true, WINO_WS_ANY, 0.0);
    if (tiles_out) *tiles_out = p.T;
    if (p.T <= 0) return 0;
    const double time = (p.nfull + WINO_SLOTS - 1) / WINO_SLOTS + (p.T > p.nfull ? wino_tail_time(p.T - p.nfull, p.split, p.nch, 0.0) : 0.0);
    return (int)(100.0 * p.T / WINO_SLOTS / time);
}

}  // namespace
