// t2d_occupancy.hip -- the occupancy grid of every env in one launch (t2d_occupancy_grid, include/t2d.h).
//
// The reference has no counterpart (its GridMapGenerator draws random grids): the rule is build-defined.  Cell (row, col) is the
// closed square of half side cell_size / 2 centred at origin + (col, row) * cell_size; it is occupied iff its Euclidean distance to
// a listed obstacle (a static ring, a participant's box or disc), as a closed filled set, is <= inflate.  tests/occupancy_ref.py
// restates the arithmetic below operation by operation; the kernel equals it bit for bit.
//
// Every element is brought to one form in phase 1: n vertices in fp64 (a ring as it is, a box as its four corners through
// sincos_det, a disc as ONE vertex whose radius is added to the threshold) with the thresholds
//     g   = 2^-44 * max(|coordinates of the element|, the window's magnitude)      the guard: rounding can only add cells
//     rg  = inflate + radius + g,  rg2 = rg * rg,  g2 = g * g
// and a cell tests, per vertex a and edge a -> b of the element,
//     (1) the vertex against the square:        max(x0 - ax, ax - x1, 0)^2 + max(y0 - ay, ay - y1, 0)^2 <= rg2
//     (2) the square's corners against the edge: 0 < t < |d|^2 and cross^2 <= rg2 |d|^2     (t, cross: of corner - a with d = b - a)
//     (3) the edge crossing the square:         the corners' crosses straddle 0 and the edge's bounding box meets the square, each
//                                               within g
// and, for a ring, (4) the cell's centre strictly inside: every cross of (centre - a) with d of one sign.  (1)-(3) are the distance
// of the ring's boundary, (4) is the cell that lies wholly inside.  No division, no square root.
//
// A workgroup (256 lanes) takes one env x one tile of kTW x kTH = 32 x 32 cells; a lane owns four neighbouring cells of one row.
// The env's elements (static rings, then participants) are walked 256 at a time:
//   phase 1  lane t takes candidate t of the batch, builds its record and tests its bounding box, grown by rg + 8 g, against the
//            tile's rectangle; survivors are appended to a list in LDS (one ballot and one LDS atomic per wave).  (1)-(4) never
//            count an element whose distance is above inflate + 4 g, so the cull drops nothing they would count.
//   phase 2  every lane tests its four cells against the list (LDS broadcast reads), after the same bounding-box test for its own
//            strip of four cells and for each cell.
// Stores are packed: two 16-byte stores of weights per lane where W is even, one dword of four mask bytes where W % 4 == 0.  The
// NAIVE instantiation skips the test of phase 1 (T2D_OCC_FORMAT_NAIVE): the yardstick of scripts/time_occupancy.py.
#include "t2d_math.h"
#include "t2d_pool.h"

namespace t2d {

namespace {

constexpr int kBlock = 256;
constexpr int kTW = 32, kTH = 32;            // cells of a tile; a lane owns 4 cells of a row: 8 lanes per row
static_assert(kTW / 4 * kTH == kBlock, "one lane per four cells");
constexpr int kMaxVerts = T2D_MAX_POLY_VERTS;
constexpr double kGuard = 0x1p-44;           // g = kGuard * magnitude

struct Rec {
    double v[2 * kMaxVerts];   // x0, y0, x1, y1, ...
    double rg2, g, g2;
    double lox, hix, loy, hiy, rc;   // the bounding box and what the cull grows it by: rg + 8 g
    int32_t n, pad;
};

// one cell against one record; (x0, x1) x (y0, y1) the square, (cx, cy) its centre
__device__ __forceinline__ bool cell_hit(const Rec& r, int n, double rg2, double g, double g2, double cx, double cy, double x0,
                                         double x1, double y0, double y1) {
    bool hit = false, anypos = false, anyneg = false, anyzero = false;
    for (int k = 0; k < n; ++k) {
        const double ax = r.v[2 * k], ay = r.v[2 * k + 1];
        const double dxv = fmax(fmax(x0 - ax, ax - x1), 0.0), dyv = fmax(fmax(y0 - ay, ay - y1), 0.0);
        hit |= dxv * dxv + dyv * dyv <= rg2;
        if (n < 3) continue;
        const int k1 = k + 1 < n ? k + 1 : 0;
        const double bx = r.v[2 * k1], by = r.v[2 * k1 + 1];
        const double dx = bx - ax, dy = by - ay;
        const double L2 = dx * dx + dy * dy, lim = rg2 * L2;
        const double ex[2] = {x0 - ax, x1 - ax}, ey[2] = {y0 - ay, y1 - ay};
        double mn = INFINITY, mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double px = ex[c & 1], py = ey[c >> 1];
            const double t = px * dx + py * dy, cr = px * dy - py * dx;
            hit |= t > 0.0 && t < L2 && cr * cr <= lim;
            mn = fmin(mn, cr); mx = fmax(mx, cr);
        }
        const double gl = g2 * L2;
        const bool lo_ok = mn <= 0.0 || mn * mn <= gl, hi_ok = mx >= 0.0 || mx * mx <= gl;
        const bool xov = x0 - fmax(ax, bx) <= g && fmin(ax, bx) - x1 <= g, yov = y0 - fmax(ay, by) <= g && fmin(ay, by) - y1 <= g;
        hit |= lo_ok && hi_ok && xov && yov;
        const double crc = (cx - ax) * dy - (cy - ay) * dx;
        if (crc > 0.0) anypos = true;
        else if (crc < 0.0) anyneg = true;
        else if (L2 != 0.0) anyzero = true;
    }
    return hit || (n >= 3 && !anyzero && anypos != anyneg);
}

template <bool NAIVE>
__global__ __launch_bounds__(kBlock) void occupancy_kernel(PoolView pv, OccView ov, double* weight, uint8_t* mask, int32_t* hw_out,
                                                           int32_t* status) {
    __shared__ Rec s_rec[kBlock];
    __shared__ int s_count, s_invalid;

    const int W = ov.W, H = ov.H;
    const int ntx = (W + kTW - 1) / kTW, ntile = ntx * ((H + kTH - 1) / kTH);
    const int e = blockIdx.x / ntile, blk = blockIdx.x % ntile;   // (e < n_env: the grid is n_env * ntile workgroups)
    const int tx = blk % ntx, ty = blk / ntx;
    const int tid = threadIdx.x, lane = tid & 63;
    const int row = ty * kTH + tid / (kTW / 4), col = tx * kTW + (tid % (kTW / 4)) * 4;
    const double cs = ov.cell_size, half = 0.5 * cs;

    // ---- this lane's four cells, and the tile's rectangle ---------------------------------------------------------------------
    const double cy = ov.origin_y + (double)row * cs, y0 = cy - half, y1 = cy + half;
    double cx[4], x0[4], x1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cx[k] = ov.origin_x + (double)(col + k) * cs;
        x0[k] = cx[k] - half; x1[k] = cx[k] + half;
    }
    const double tx0 = (ov.origin_x + (double)(tx * kTW) * cs) - half, tx1 = (ov.origin_x + (double)(min(tx * kTW + kTW, W) - 1) * cs) + half;
    const double ty0 = (ov.origin_y + (double)(ty * kTH) * cs) - half, ty1 = (ov.origin_y + (double)(min(ty * kTH + kTH, H) - 1) * cs) + half;

    // ---- the env's candidates: [static rings][participants] --------------------------------------------------------------------
    int n_static = 0, s0 = 0;
    const bool scene = ov.scene_quads != nullptr;
    if (scene) n_static = max(0, min(ov.scene_n_quads[e], (int)T2D_GEN_MAX_QUADS));
    else if (ov.env_poly_off) { s0 = ov.env_poly_off[e]; n_static = ov.env_poly_off[e + 1] - s0; }
    const int total = n_static + (ov.include_participants ? pv.A : 0);

    bool occ[4] = {false, false, false, false};
    if (tid == 0) s_invalid = 0;

    for (int base = 0; base < total; base += kBlock) {
        if (tid == 0) s_count = 0;
        __syncthreads();
        // ---- phase 1: lane t <- candidate base + t ----------------------------------------------------------------------------
        const int i = base + tid;
        Rec r;
        r.n = 0; r.pad = 0;
        bool hit = false;
        if (i < total) {
            int n = 0;
            double rad = 0.0, mag = ov.mwin;
            if (i >= n_static) {   // a participant: its oriented box, or the disc of a T2D_SHAPE_CIRCLE type
                const int a = i - n_static, idx = e * pv.A + a;
                const uint32_t ids = pv.ids[idx];
                if (((ids >> kIdsActiveShift) & 0xffu) && a != ov.exclude_slot) {
                    const int type = (ids >> kIdsTypeShift) & (T2D_MAX_TYPES - 1);
                    const float xf = pv.x[idx], yf = pv.y[idx], hf = pv.heading[idx];
                    if (!(__builtin_isfinite(xf) && __builtin_isfinite(yf) && __builtin_isfinite(hf))) {
                        s_invalid = 1;   // (every writer stores the same value)
                    } else {
                        const double x = (double)xf, y = (double)yf;
                        const double L = pv.params[T2D_P_LENGTH * T2D_MAX_TYPES + type], Wd = pv.params[T2D_P_WIDTH * T2D_MAX_TYPES + type];
                        if ((int)pv.params[T2D_P_SHAPE * T2D_MAX_TYPES + type] == T2D_SHAPE_CIRCLE) {
                            n = 1;
                            rad = fmax(0.5 * Wd, 0.0);
                            r.v[0] = x; r.v[1] = y;
                            mag = fmax(mag, rad);
                        } else {
                            n = 4;
                            double s, c;
                            sincos_det((double)hf, s, c);
                            const double hl = 0.5 * L, hwd = 0.5 * Wd;
                            const double lx[4] = {hl, hl, -hl, -hl}, ly[4] = {-hwd, hwd, hwd, -hwd};
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                r.v[2 * k] = x + (lx[k] * c - ly[k] * s);
                                r.v[2 * k + 1] = y + (lx[k] * s + ly[k] * c);
                            }
                        }
                    }
                }
            } else {               // a static ring, undivided
                const float* src;
                n = 4;
                if (scene) {
                    src = ov.scene_quads + ((size_t)e * T2D_GEN_MAX_QUADS + i) * 8;
                    if (ov.scene_quad_id[(size_t)e * T2D_GEN_MAX_QUADS + i] < 0) n = 0;
                } else {
                    const int v0 = ov.poly_vert_off[s0 + i];
                    n = ov.poly_vert_off[s0 + i + 1] - v0;
                    src = ov.poly_xy + 2 * (size_t)v0;
                }
                n = n > kMaxVerts ? kMaxVerts : n;   // (the library admits rings of 3 .. T2D_MAX_POLY_VERTS vertices: never taken)
                if (n < 3) n = 0;
#pragma unroll
                for (int k = 0; k < kMaxVerts; ++k) {
                    if (k >= n) break;
                    r.v[2 * k] = (double)src[2 * k]; r.v[2 * k + 1] = (double)src[2 * k + 1];
                }
            }
            if (n > 0) {
                double lox = INFINITY, hix = -INFINITY, loy = INFINITY, hiy = -INFINITY;
#pragma unroll
                for (int k = 0; k < kMaxVerts; ++k) {
                    if (k >= n) break;
                    const double x = r.v[2 * k], y = r.v[2 * k + 1];
                    lox = fmin(lox, x); hix = fmax(hix, x); loy = fmin(loy, y); hiy = fmax(hiy, y);
                    mag = fmax(mag, fmax(fabs(x), fabs(y)));
                }
                const double g = mag * kGuard, rg = (ov.inflate + rad) + g;
                r.n = n; r.g = g; r.g2 = g * g; r.rg2 = rg * rg;
                const double rc = rg + 8.0 * g;
                r.lox = lox; r.hix = hix; r.loy = loy; r.hiy = hiy; r.rc = rc;
                hit = NAIVE || (lox - tx1 <= rc && tx0 - hix <= rc && loy - ty1 <= rc && ty0 - hiy <= rc);
            }
        }
        // append: one ballot and one LDS atomic per wave
        const unsigned long long hits = __ballot(hit);
        int wave_base = 0;
        if (lane == 0 && hits != 0ull) wave_base = atomicAdd(&s_count, __builtin_popcountll(hits));
        wave_base = __shfl(wave_base, 0);
        if (hit) s_rec[wave_base + __builtin_popcountll(hits & ((1ull << lane) - 1ull))] = r;
        __syncthreads();
        // ---- phase 2: four cells against the list ---------------------------------------------------------------------------------
        const int count = s_count;
        for (int j = 0; j < count; ++j) {
            const Rec& q = s_rec[j];
            const int n = q.n;
            const double rg2 = q.rg2, g = q.g, g2 = q.g2;
            // the cull of phase 1 again, for this lane's strip and then per cell (the product form only)
            const double rc = q.rc, lox = q.lox, hix = q.hix;
            if (!NAIVE && !(q.loy - y1 <= rc && y0 - q.hiy <= rc && lox - x1[3] <= rc && x0[0] - hix <= rc)) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (!occ[k] && (NAIVE || (lox - x1[k] <= rc && x0[k] - hix <= rc)))
                    occ[k] = cell_hit(q, n, rg2, g, g2, cx[k], cy, x0[k], x1[k], y0, y1);
        }
        __syncthreads();
    }
    if (total <= 0) __syncthreads();   // (s_invalid = 0 of lane 0)
    const bool invalid = s_invalid != 0;
    if (invalid) occ[0] = occ[1] = occ[2] = occ[3] = true;

    // ---- stores -------------------------------------------------------------------------------------------------------------------
    if (blk == 0 && tid == 0) {
        if (hw_out) { hw_out[2 * e] = H; hw_out[2 * e + 1] = W; }
        if (status) status[e] = invalid ? T2D_OCC_INVALID : T2D_OCC_OK;
    }
    if (row >= H || col >= W) return;
    const size_t cell = ((size_t)e * H + row) * W + col;
    double wv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) wv[k] = occ[k] ? INFINITY : ov.free_weight;
    if (weight) {
        if ((W & 1) == 0) {   // (col is a multiple of four and W is even: the pairs are inside or outside together, and 16-byte aligned)
            *reinterpret_cast<double2*>(weight + cell) = make_double2(wv[0], wv[1]);
            if (col + 2 < W) *reinterpret_cast<double2*>(weight + cell + 2) = make_double2(wv[2], wv[3]);
        } else {
            for (int k = 0; k < 4 && col + k < W; ++k) weight[cell + k] = wv[k];
        }
    }
    if (mask) {
        if ((W & 3) == 0) {
            *reinterpret_cast<uint32_t*>(mask + cell) = (uint32_t)occ[0] | (uint32_t)occ[1] << 8 | (uint32_t)occ[2] << 16 | (uint32_t)occ[3] << 24;
        } else {
            for (int k = 0; k < 4 && col + k < W; ++k) mask[cell + k] = (uint8_t)occ[k];
        }
    }
}

}  // namespace

hipError_t launch_occupancy(const PoolView& v, const OccView& ov, double* weight, uint8_t* mask, int32_t* hw, int32_t* status, int naive,
                            hipStream_t s) {
    const int ntx = (ov.W + kTW - 1) / kTW, nty = (ov.H + kTH - 1) / kTH;
    const dim3 grid((unsigned)(ntx * nty) * (unsigned)v.n_env);   // (t2d_occupancy_grid bounds the product)
    if (naive) hipLaunchKernelGGL(occupancy_kernel<true>, grid, dim3(kBlock), 0, s, v, ov, weight, mask, hw, status);
    else hipLaunchKernelGGL(occupancy_kernel<false>, grid, dim3(kBlock), 0, s, v, ov, weight, mask, hw, status);
    return hipGetLastError();
}

}  // namespace t2d
