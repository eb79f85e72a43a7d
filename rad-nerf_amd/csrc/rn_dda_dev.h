// rn_dda_dev.h -- the occupancy-grid DDA walk: ONE loop (Dda::walk) with a sink per use (count / emit / record), the jittered
// start and the per-slot march of the inference loop.  Shared by the marching kernels of rn_raymarching.hip and the
// device-side inference loop of rn_head_loop.hip (identical samples from both).
#pragma once

#include "rn_common.h"

#include <float.h>

namespace rn {

constexpr float kSqrt3 = 1.7320508075688772f;

// The DDA shared by the three marching kernels (raymarching.cu:400-441 == 466-517 == 875-928).

// raymarching.cu:42-54.  frexpf/scalbnf are exact on every target, so `level` is bit-exact.
__device__ __forceinline__ int mip_from_pos(float x, float y, float z, float max_cascade) {
    const float mx = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
    int e;
    frexpf(mx, &e);
    return (int)fminf(max_cascade - 1, fmaxf(0.0f, (float)e));
}
__device__ __forceinline__ int mip_from_dt(float dt, float H, float max_cascade) {
    const float mx = (float)((double)(dt * H) * 0.5);
    int e;
    frexpf(mx, &e);
    return (int)fminf(max_cascade - 1, fmaxf(0.0f, (float)e));
}

struct Dda {
    float ox, oy, oz, dx, dy, dz, rdx, rdy, rdz;
    float rH, H3, bound, dt_gamma, dt_min, dt_max, far, Cf, Hf;
    float mb1, rmb1;  // one cascade: mip_bound = min(2^0, bound) and its reciprocal are the same for every lattice point
    bool one_cascade;
    bool one_step_skips;  // see init()
    bool span = false;    // walk<true>() tests lattice points in [t_lo, t_hi) only: set by set_span(), off for everyone else
    float t_lo = 0.0f, t_hi = 0.0f;
    uint32_t H;
    const uint8_t *grid;

    __device__ __forceinline__ void init(const float *o, const float *d, float bound_, float dt_gamma_,
                                         uint32_t max_steps, uint32_t C, uint32_t H_, const uint8_t *grid_,
                                         float far_) {
        ox = o[0]; oy = o[1]; oz = o[2];
        dx = d[0]; dy = d[1]; dz = d[2];
        rdx = 1 / dx; rdy = 1 / dy; rdz = 1 / dz;
        H = H_; Hf = (float)H_; Cf = (float)C;
        rH = 1 / Hf;
        H3 = (float)(H_ * H_ * H_);
        bound = bound_; dt_gamma = dt_gamma_; far = far_; grid = grid_;
        dt_max = 2 * kSqrt3 * (float)(1 << (C - 1)) / Hf;        // :386
        dt_min = fminf(dt_max, 2 * kSqrt3 / (float)max_steps);   // :387
        mb1 = fminf(1.0f, bound_);
        rmb1 = 1 / mb1;
        one_cascade = C == 1 && H_ <= 256;  // then level * H3 + (float)morton < 2^24 is exact: no float round trip needed
        // An empty cell is left by `do t += dt while (t < tt)` with tt = the cell's exit time (:430-440).  With ONE cascade and
        // dt_min == dt_max (max_steps <= H: every configuration of this repo) dt is the constant 2 sqrt(3) / H = the cell's
        // diagonal, while the ray stays in a cell for at most (cell side) / max|d_i| <= (2 / H) / max|d_i|.  For max|d_i| > 0.58
        // (all rays but those within 0.3 deg of a space diagonal) that is < 0.9955 dt: the loop body runs exactly once whatever
        // tx, ty, tz round to, so the 30-odd operations that compute them are skipped.  Same t, same samples, bit for bit.
        one_step_skips = C == 1 && dt_min == dt_max && fmaxf(fabsf(dx), fmaxf(fabsf(dy), fabsf(dz))) > 0.58f;
    }

    // The occupied box's span (opt-in; the inference loop's marchers call it after init()).  box = {lo[3], hi[3]}: the cell
    // coordinates between which every set bit of cascade 0 lies (rn_occ_box; lo > hi: no bit is set).
    //
    // t advances by t += clampf(t * dt_gamma, dt_min, dt_max) whatever the grid holds, and on a one_step_skips ray every lattice
    // point is tested on its own: it is a sample iff its cell's bit is set.  A point whose cell lies outside the box has no bit
    // set, so not testing it changes no sample, no count and no t.  [t_lo, t_hi] is the slab test of the ray against the box
    // GROWN BY ONE WHOLE CELL on every side: at t < t_lo (t >= t_hi) the point has not entered (has left) the grown slab of some
    // axis, i.e. it is a whole cell -- 2 mb1 / H -- away from the box on that axis, while everything that rounds between the
    // slab's face and the point's cell (the face, face - o, 1 / d, the product, o + t * d, the cell coordinate) is off by less than
    // 8 * 2^-24 (|o| + 2 mb1): under a tenth of a cell for H <= 256 (one_cascade) and |o_i| <= 4096 mb1, which set_span() requires.
    // Every other ray keeps the full walk: more than one cascade, variable dt, max|d_i| <= 0.58, a far origin, a span that
    // overflowed.  A NaN never narrows the span: fmaxf / fminf return their other operand.
    //
    // One axis: the slab of cells lo - 1 .. hi + 1 in world coordinates narrows [a, b].  A side on which the box reaches the
    // grid's border has no face (cell_of() clamps every point beyond onto the border cells).  A ray that does not move on the
    // axis (d == 0: o + t * d is o for every finite t) is inside or outside by its origin alone.
    __device__ __forceinline__ void span_axis(float o, float d, float rd, int lo, int hi, float &a, float &b) const {
        const bool open_lo = lo <= 0, open_hi = hi >= (int)H - 1;
        const float f_lo = ((float)(lo - 1) * rH * 2 - 1) * mb1, f_hi = ((float)(hi + 2) * rH * 2 - 1) * mb1;
        if (d == 0.0f) {
            if ((!open_lo && o < f_lo) || (!open_hi && o > f_hi)) { a = FLT_MAX; b = -FLT_MAX; }
            return;
        }
        const float t_f_lo = (f_lo - o) * rd, t_f_hi = (f_hi - o) * rd;
        if (d > 0.0f) {
            if (!open_lo) a = fmaxf(a, t_f_lo);
            if (!open_hi) b = fminf(b, t_f_hi);
        } else {
            if (!open_hi) a = fmaxf(a, t_f_hi);
            if (!open_lo) b = fminf(b, t_f_lo);
        }
    }
    __device__ __forceinline__ void set_span(const int32_t *__restrict__ box) {
        if (!(one_cascade && one_step_skips)) return;
        if (!(fmaxf(fabsf(ox), fmaxf(fabsf(oy), fabsf(oz))) <= 4096.0f * mb1)) return;
        float a = -FLT_MAX, b = FLT_MAX;
        span_axis(ox, dx, rdx, box[0], box[3], a, b);
        span_axis(oy, dy, rdy, box[1], box[4], a, b);
        span_axis(oz, dz, rdz, box[2], box[5], a, b);
        if (!(fabsf(a) <= FLT_MAX && fabsf(b) <= FLT_MAX)) return;   // overflowed: the full walk
        t_lo = a; t_hi = b; span = true;
    }

    // occupancy-grid cell of the lattice point at parameter t (raymarching.cu:404-419); returns the bit index.
    //
    // :415-417 spell the cell coordinate as 0.5 * (double)(x * mip_rbound + 1) * (double)H, narrowed to float by
    // clamp().  v = x * mip_rbound + 1 has 24 significant bits and H < 2^24, so the double product v * H / 2 is exact
    // and its narrowing is the correctly rounded value of v * H / 2 -- which is what the single fp32 multiply
    // v * (0.5f * H) returns (0.5 * H is exact).  Same bits, no fp64.  With one cascade the level is 0 for every point.
    __device__ __forceinline__ uint32_t cell_of(float t, float &x, float &y, float &z, float &dt, float &mip_bound, int &nx,
                                                int &ny, int &nz) const {
        x = clampf(ox + t * dx, -bound, bound);
        y = clampf(oy + t * dy, -bound, bound);
        z = clampf(oz + t * dz, -bound, bound);
        dt = clampf(t * dt_gamma, dt_min, dt_max);
        if (one_cascade) {  // wave-uniform fast path: same arithmetic with the per-ray constants hoisted (level = 0)
            mip_bound = mb1;
            const float half_h1 = 0.5f * Hf, top1 = (float)(H - 1);
            nx = (int)clampf((x * rmb1 + 1) * half_h1, 0.0f, top1);
            ny = (int)clampf((y * rmb1 + 1) * half_h1, 0.0f, top1);
            nz = (int)clampf((z * rmb1 + 1) * half_h1, 0.0f, top1);
            return morton3D_8((uint32_t)nx, (uint32_t)ny, (uint32_t)nz);    // one_cascade implies H <= 256
        }
        int level = 0;
        if (Cf > 1.0f) {  // wave-uniform
            const int lp = mip_from_pos(x, y, z, Cf), ld = mip_from_dt(dt, Hf, Cf);
            level = lp > ld ? lp : ld;
        }
        mip_bound = fminf(scalbnf(1.0f, level), bound);
        const float mip_rbound = 1 / mip_bound;
        const float half_h = 0.5f * Hf, top = (float)(H - 1);
        nx = (int)clampf((x * mip_rbound + 1) * half_h, 0.0f, top);
        ny = (int)clampf((y * mip_rbound + 1) * half_h, 0.0f, top);
        nz = (int)clampf((z * mip_rbound + 1) * half_h, 0.0f, top);
        // :419 -- evaluated in float (H3 is a float in the reference)
        return (uint32_t)((float)level * H3 + (float)morton3D((uint32_t)nx, (uint32_t)ny, (uint32_t)nz));
    }

    // Walk from t, at most `limit` occupied steps; sink(*this, step, t, x, y, z, dt) sees every sample (see the sinks below).
    // (Measured on MI355X: the walk is bound by its own arithmetic, ~100 VALU ops per lattice point, not by the
    // dependent bitfield loads -- fetching the occupancy of the next 4 / 8 / 16 lattice points together and replaying the
    // decisions on a bit mask made k_head_march 10-17 % slower, so the loop keeps the reference's shape.)
    // SPAN (opt-in, see set_span()): on lanes with `span` the lattice points before t_lo are stepped over by the loop's own
    // t += dt without a cell or a load, and the walk ends at t_hi; the guard counts the stepped-over points too.
    // AHEAD (opt-in, with SPAN): on lanes with `span` -- one cascade, one_step_skips, so the lattice point after t is t + dt whatever
    // the grid holds -- the occupancy byte of the NEXT point is asked for before the current point's is looked at: its round trip
    // passes under the current point's decision and the next point's arithmetic.  Same points, same tests, same order; the one
    // byte read past the walk's last point lies in the grid like every other (cell_of() clamps the cell).
    template <bool SPAN = false, bool AHEAD = false, class Sink>
    __device__ __forceinline__ uint32_t walk(float &t_io, uint32_t limit, Sink sink) const {
        float t = t_io;
        uint32_t step = 0;
        uint32_t guard = 0;  // not in the reference: bounds the walk on degenerate inputs (far = inf)
        float end = far;
        if constexpr (SPAN) {
            if (span) {
                end = t_hi < far ? t_hi : far;               // a NaN far stays: no t is below it, as in the full walk
                const float first = t_lo < end ? t_lo : end;
                while (t < first && guard < (1u << 20)) {
                    t += clampf(t * dt_gamma, dt_min, dt_max);
                    guard++;
                }
                if constexpr (AHEAD) {
                    // two points in flight, A and B by turns (no register is copied, so no copy waits for a byte on its way);
                    // inside the loop the next point is fetched whether or not the walk will get to it
                    if (!(t < end && limit > 0u)) { t_io = t; return 0u; }   // an empty span: nothing is fetched
                    float xa, ya, za, dta, xb, yb, zb, dtb, mip_bound;
                    int nx, ny, nz;
                    uint32_t ia = cell_of(t, xa, ya, za, dta, mip_bound, nx, ny, nz), ib;
                    uint32_t ba = grid[ia >> 3], bb;
                    for (;;) {
                        if (!(t < end && step < limit && guard < (1u << 20))) break;
                        const float tb = t + dta;
                        ib = cell_of(tb, xb, yb, zb, dtb, mip_bound, nx, ny, nz);
                        bb = grid[ib >> 3];
                        if (ba & (1u << (ia & 7u))) { sink(*this, step, t, xa, ya, za, dta); step++; } else { guard++; }
                        guard++;
                        t = tb;
                        if (!(t < end && step < limit && guard < (1u << 20))) break;
                        const float ta = t + dtb;
                        ia = cell_of(ta, xa, ya, za, dta, mip_bound, nx, ny, nz);
                        ba = grid[ia >> 3];
                        if (bb & (1u << (ib & 7u))) { sink(*this, step, t, xb, yb, zb, dtb); step++; } else { guard++; }
                        guard++;
                        t = ta;
                    }
                    t_io = t;
                    return step;
                }
            }
        }
        while (t < (SPAN ? end : far) && step < limit && guard < (1u << 20)) {
            float x, y, z, dt, mip_bound;
            int nx, ny, nz;
            const uint32_t index = cell_of(t, x, y, z, dt, mip_bound, nx, ny, nz);
            if (grid[index >> 3] & (1u << (index & 7u))) {
                sink(*this, step, t, x, y, z, dt);
                t += dt;
                step++;
            } else if (one_step_skips) {
                t += dt;                     // = t + clampf(t * dt_gamma, dt_min, dt_max), the loop's single pass
                guard++;
            } else {
                const float sx = copysignf(1.0f, dx), sy = copysignf(1.0f, dy), sz = copysignf(1.0f, dz);
                const float tx = ((((float)nx + 0.5f + 0.5f * sx) * rH * 2 - 1) * mip_bound - x) * rdx;
                const float ty = ((((float)ny + 0.5f + 0.5f * sy) * rH * 2 - 1) * mip_bound - y) * rdy;
                const float tz = ((((float)nz + 0.5f + 0.5f * sz) * rH * 2 - 1) * mip_bound - z) * rdz;
                // Clipping the cell-exit time at `far` changes no output: once t >= far the walk is over.
                const float tt = fminf(t + fmaxf(0.0f, fminf(tx, fminf(ty, tz))), far);
                do {
                    t += clampf(t * dt_gamma, dt_min, dt_max);
                    guard++;
                } while (t < tt && guard < (1u << 20));
            }
            guard++;
        }
        t_io = t;
        return step;
    }

    // The sinks of walk().  CountSamples: the count is all the caller wants.
    struct CountSamples {
        __device__ __forceinline__ void operator()(const Dda &, uint32_t, float, float, float, float, float) {}
    };
    // EmitSamples: sample k goes to row k of xyzs / dirs / deltas; deltas = (dt, t of the next lattice point).
    struct EmitSamples {
        float *xyzs, *dirs, *deltas;
        __device__ __forceinline__ void operator()(const Dda &s, uint32_t, float t, float x, float y, float z, float dt) {
            xyzs[0] = x; xyzs[1] = y; xyzs[2] = z;
            dirs[0] = s.dx; dirs[1] = s.dy; dirs[2] = s.dz;
            deltas[0] = dt;
            deltas[1] = t + dt;
            xyzs += 3; dirs += 3; deltas += 2;
        }
    };
    // RecordSamples: remember where each sample was taken instead of writing it, rec[k * stride] = t of sample k; emit()
    // rebuilds the sample from that t -- same bits -- so a caller that must know every ray's count before it can place the
    // samples (the training marcher) walks once, not twice.
    struct RecordSamples {
        float *rec;
        uint32_t stride;
        __device__ __forceinline__ void operator()(const Dda &, uint32_t step, float t, float, float, float, float) { rec[step * stride] = t; }
    };

    // the sample at parameter t, as walk() hands it to EmitSamples (the expressions of cell_of())
    __device__ __forceinline__ void emit(float t, float *xyz, float *dir, float *delta) const {
        EmitSamples{xyz, dir, delta}(*this, 0u, t, clampf(ox + t * dx, -bound, bound), clampf(oy + t * dy, -bound, bound),
                                     clampf(oz + t * dz, -bound, bound), clampf(t * dt_gamma, dt_min, dt_max));
    }

    // the jittered start of a ray whose walk begins at t (raymarching.cu:392 == :873): u = a uniform number, 0 = no jitter
    __device__ __forceinline__ float start(float t, float u) const { return t + clampf(t * dt_gamma, dt_min, dt_max) * u; }

    // One ray's share of a loop iteration: at most n_step samples from t into rows base .. base + n_step - 1; the rows the walk
    // did not reach get deltas = 0 (the network and the compositor skip them), so the sample buffers never need a memset.
    // t is taken by value: where the walk stops is not visible to anyone (the compositor writes rays_t from deltas), which is
    // what lets SPAN end a walk at t_hi instead of far.
    // EXP: experiment only (the RN_EXP_LOOP_* switches of rn_head_loop.hip, 0 in every build that renders): kExpNoStores -- the
    // walk without its sample stores; kExpNoFill -- without the zero fill; kExpNoWalk -- no lattice point is tested.
    static constexpr int kExpNoStores = 1, kExpNoFill = 2, kExpNoWalk = 4;
    template <bool SPAN = false, int EXP = 0, bool AHEAD = false>
    __device__ __forceinline__ uint32_t march_slot(float t, uint32_t n_step, uint32_t base, float *xyzs, float *dirs, float *deltas) const {
        const uint32_t limit = (EXP & kExpNoWalk) ? 0u : n_step;
        uint32_t emitted;
        if constexpr ((EXP & kExpNoStores) != 0) emitted = walk<SPAN, AHEAD>(t, limit, CountSamples{});
        else emitted = walk<SPAN, AHEAD>(t, limit, EmitSamples{xyzs + (size_t)base * 3, dirs + (size_t)base * 3, deltas + (size_t)base * 2});
        if constexpr ((EXP & kExpNoFill) == 0)
            for (uint32_t k = emitted; k < n_step; k++) { deltas[((size_t)base + k) * 2] = 0.0f; deltas[((size_t)base + k) * 2 + 1] = 0.0f; }
        return emitted;
    }
};

}  // namespace rn
