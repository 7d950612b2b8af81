// t2d_camera.hip -- the BEV camera of every env in one launch (t2d_camera_render, include/t2d.h).
//
// Replaces (reference, tactics2d v0.1.9rc3):
//   BEVCamera._get_map_elements / _get_participants   sensor/camera.py:89-331       what is listed, in which order
//   MatplotlibRenderer._calculate_bounds / auto_scale renderer/matplotlib_renderer.py:137-232   the view window
//   MatplotlibRenderer._transform_to_camera_view      :435-460   v = R(+camera_yaw) (p - sensor) + sensor
//   MatplotlibRenderer._resolve_style                 :234-286   colour and z-order of a class
// The raster itself is build-defined: pixel (r, c) = the class of the topmost element that contains the
// CENTRE of the pixel, row 0 at the front edge; even-odd crossing on the undivided ring, dx^2 + dy^2 <= r^2 for circles; no
// anti-aliasing, no outline strokes, no road lines.
//
// A workgroup (256 lanes) takes one env x one block of kBW x kBH = 64 x 16 pixels; a lane owns four neighbouring pixels of
// one row, whose centres it takes to the WORLD frame once (fp32: offset from the sensor, then one rotation) -- elements are
// never transformed per pixel.  The env's elements (target area, static rings, lane rings, track tiles, participants) are
// walked 256 at a time:
//   phase 1  lane t takes candidate t of the batch, brings its vertices to the camera frame (one rotation per vertex, once
//            per block) and tests their bounding box against the block's rectangle; survivors are appended to a list in
//            LDS (one ballot and one LDS atomic per wave; a body and its heading triangle share a record).  Their order in the list does not matter: every record carries
//            its draw key z << 24 | listing position, and "topmost" is the largest key (equal z: the later listing wins,
//            what matplotlib's stable sort of the artists does).
//   phase 2  every lane tests its four pixels against the short list (LDS broadcast reads) and keeps the class of the largest
//            key.
// Stores are packed: one dword of four class bytes and three dwords of four RGB pixels per lane (rows of a width that is
// not a multiple of four fall back to byte stores).  The NAIVE instantiation skips the test of phase 1 -- every pixel then
// tests every element: the yardstick of scripts/camera_probe.py (T2D_CAMERA_FORMAT_NAIVE).
#include "t2d_math.h"
#include "t2d_pool.h"

namespace t2d {

namespace {

constexpr int kBlock = 256;
constexpr int kBW = 64, kBH = 16;            // pixels of a block; a lane owns 4 pixels of a row: 16 lanes per row
static_assert(kBW / 4 * kBH == kBlock, "one lane per four pixels");
constexpr int kMaxVerts = T2D_MAX_POLY_VERTS;   // vertices of a ring (the library's limit for caller polygons)
constexpr float kCullMargin = 1e-2f;         // m: the bounding-box test of phase 1 is widened by this much (fp32 rounding of
                                             // the rotation is of the order of 1e-4 m at a few hundred metres)

enum { kPolygon = 0, kBox = 1, kTriangle = 2, kCircle = 3 };

// One listed element in LDS.  polygon: v = x0, y0, x1, y1, ... (world frame); box / triangle: v = {x, y, cos h, sin h, half
// length, half width}; circle: v = {x, y, r^2}
struct Rec {
    uint32_t key;       // z << 24 | listing position (group << 20 | index)
    uint32_t kind_n;    // kind | n_vertices << 8 | class << 16
    float v[2 * kMaxVerts];
};

__device__ __forceinline__ bool in_polygon(const float* v, int n, float px, float py) {
    bool in = false;
    float x1 = v[2 * n - 2], y1 = v[2 * n - 1];
    for (int k = 0; k < n; ++k) {
        const float x2 = v[2 * k], y2 = v[2 * k + 1];
        if ((y1 > py) != (y2 > py)) {
            // px < x1 + (x2 - x1) (py - y1) / (y2 - y1), without the division
            const float d = y2 - y1;
            const float lhs = (px - x1) * d, rhs = (x2 - x1) * (py - y1);
            in ^= d > 0.f ? lhs < rhs : lhs > rhs;
        }
        x1 = x2; y1 = y2;
    }
    return in;
}

__device__ __forceinline__ bool rec_contains(const Rec& r, int kind, int n, float px, float py) {
    if (kind == kPolygon) return in_polygon(r.v, n, px, py);
    const float dx = px - r.v[0], dy = py - r.v[1];
    if (kind == kCircle) return dx * dx + dy * dy <= r.v[2];
    const float bx = dx * r.v[2] + dy * r.v[3], by = dy * r.v[2] - dx * r.v[3];   // body frame
    const float hl = r.v[4], hw = r.v[5];
    if (kind == kBox) return fabsf(bx) <= hl && fabsf(by) <= hw;
    return bx >= 0.f && bx * hw + fabsf(by) * hl <= hl * hw;   // (hl, 0), (0, hw), (0, -hw)
}

template <bool NAIVE>
__global__ __launch_bounds__(kBlock) void camera_kernel(PoolView pv, CameraView cv, TrackView tv, uint8_t* out_class, uint8_t* out_rgb) {
    __shared__ Rec s_rec[kBlock];   // (a body and its heading arrow share a record)
    __shared__ int s_count;

    const int W = cv.width, H = cv.height;
    const int nbx = (W + kBW - 1) / kBW, nblk = nbx * ((H + kBH - 1) / kBH);
    const int e = blockIdx.x / nblk, blk = blockIdx.x % nblk;   // (e < n_env: the grid is n_env * nblk workgroups)
    const int bx = blk % nbx, by = blk / nbx;
    const int tid = threadIdx.x, lane = tid & 63;
    const int row = by * kBH + tid / (kBW / 4), col = bx * kBW + (tid % (kBW / 4)) * 4;

    // ---- the sensor: the bound participant's pose --------------------------------------------------------------------------
    const int bidx = e * pv.A + cv.bind_slot;
    const float sx = pv.x[bidx], sy = pv.y[bidx], sh = pv.heading[bidx];
    const bool sane = __builtin_isfinite(sx) && __builtin_isfinite(sy) && __builtin_isfinite(sh);
    // camera_yaw = pi / 2 - heading (the agent points to the front) or 0: cos(yaw) = sin h, sin(yaw) = cos h
    float cyaw = 1.f, syaw = 0.f;
    if (cv.heading_up && sane) {
        double s, c;
        sincos_det((double)sh, s, c);
        cyaw = (float)s; syaw = (float)c;
    }

    // ---- this lane's four pixel centres, in the world frame: p = sensor + R(-yaw) u ------------------------------------------
    float wx[4], wy[4];
    {
        const float uy = cv.uy1 - ((float)row + 0.5f) * cv.px_h;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float ux = cv.ux0 + ((float)(col + k) + 0.5f) * cv.px_w;
            wx[k] = sx + (ux * cyaw + uy * syaw);
            wy[k] = sy + (uy * cyaw - ux * syaw);
        }
    }
    // the block's rectangle in the camera frame (offsets from the sensor), pixel centres, widened
    const float rx0 = cv.ux0 + ((float)(bx * kBW) + 0.5f) * cv.px_w - kCullMargin;
    const float rx1 = cv.ux0 + ((float)(min(bx * kBW + kBW, W) - 1) + 0.5f) * cv.px_w + kCullMargin;
    const float ry1 = cv.uy1 - ((float)(by * kBH) + 0.5f) * cv.px_h + kCullMargin;
    const float ry0 = cv.uy1 - ((float)(min(by * kBH + kBH, H) - 1) + 0.5f) * cv.px_h - kCullMargin;

    // ---- the env's candidates: [target][static rings][lane rings][track tiles][participants] -----------------------------
    const int n_target = (cv.layers & T2D_CAMERA_LAYER_TARGET) && pv.target_xy ? 1 : 0;
    int n_static = 0, s0 = 0;
    const bool scene = cv.scene_quads != nullptr;
    if (cv.layers & T2D_CAMERA_LAYER_STATIC) {
        if (scene) n_static = max(0, min(cv.scene_n_quads[e], (int)T2D_GEN_MAX_QUADS));
        else if (cv.env_poly_off[0]) { s0 = cv.env_poly_off[0][e]; n_static = cv.env_poly_off[0][e + 1] - s0; }
    }
    int n_lane = 0, l0 = 0;
    if ((cv.layers & T2D_CAMERA_LAYER_LANES) && cv.env_poly_off[1]) { l0 = cv.env_poly_off[1][e]; n_lane = cv.env_poly_off[1][e + 1] - l0; }
    int n_tile = 0, t0 = 0;
    if ((cv.layers & T2D_CAMERA_LAYER_TRACKS) && tv.installed) {
        const int set = tv.set_of_env[e];
        t0 = tv.set_start[set];
        n_tile = tv.n_tile[set];
    }
    const int n_part = (cv.layers & T2D_CAMERA_LAYER_PARTICIPANTS) ? pv.A : 0;
    const int b1 = n_target, b2 = b1 + n_static, b3 = b2 + n_lane, b4 = b3 + n_tile, total = sane ? b4 + n_part : 0;

    uint32_t best_key[4] = {0u, 0u, 0u, 0u};
    uint32_t best_cls[4] = {T2D_CAMERA_CLASS_BACKGROUND, T2D_CAMERA_CLASS_BACKGROUND, T2D_CAMERA_CLASS_BACKGROUND, T2D_CAMERA_CLASS_BACKGROUND};

    for (int base = 0; base < total; base += kBlock) {
        if (tid == 0) s_count = 0;
        __syncthreads();
        // ---- phase 1: lane t <- candidate base + t --------------------------------------------------------------------
        const int i = base + tid;
        Rec r;
        r.key = 0u; r.kind_n = 0u;
        bool hit = false, arrow = false;
        int cls = 0;
        if (i < total) {
            int kind = kPolygon, n = 4;
            uint32_t listing;
            if (i >= b4) {   // a participant: Vehicle / Cyclist = body ring + heading triangle, Pedestrian = circle (camera.py:251-319)
                const int a = i - b4, idx = e * pv.A + a;
                const uint32_t ids = pv.ids[idx];
                const int type = (ids >> kIdsTypeShift) & (T2D_MAX_TYPES - 1);   // (t2d_reset admits only rows of the table)
                const float x = pv.x[idx], y = pv.y[idx], h = pv.heading[idx];
                cls = cv.class_of_type[type];
                listing = 3u << 20 | (uint32_t)(2 * a);
                if (((ids >> kIdsActiveShift) & 0xffu) && cls != T2D_CAMERA_CLASS_BACKGROUND && __builtin_isfinite(x) && __builtin_isfinite(y) &&
                    __builtin_isfinite(h)) {
                    const float L = (float)pv.params[T2D_P_LENGTH * T2D_MAX_TYPES + type], Wd = (float)pv.params[T2D_P_WIDTH * T2D_MAX_TYPES + type];
                    r.v[0] = x; r.v[1] = y;
                    float reach;
                    if ((int)pv.params[T2D_P_SHAPE * T2D_MAX_TYPES + type] == T2D_SHAPE_CIRCLE) {
                        kind = kCircle; n = 0;
                        const float rad = fmaxf(0.5f * Wd, 0.f);
                        r.v[2] = rad * rad;
                        reach = rad;
                    } else {
                        kind = kBox; n = 0;
                        double s, c;
                        sincos_det((double)h, s, c);
                        r.v[2] = (float)c; r.v[3] = (float)s; r.v[4] = 0.5f * L; r.v[5] = 0.5f * Wd;
                        reach = sqrtf(r.v[4] * r.v[4] + r.v[5] * r.v[5]);
                        arrow = (cv.layers & T2D_CAMERA_LAYER_ARROWS) != 0;
                    }
                    // (a disc around the centre bounds every orientation: cheaper than four corners, and nearly as tight)
                    const float dx = x - sx, dy = y - sy;
                    const float ux = dx * cyaw - dy * syaw, uy = dx * syaw + dy * cyaw;
                    hit = NAIVE || (ux + reach >= rx0 && ux - reach <= rx1 && uy + reach >= ry0 && uy - reach <= ry1);
                }
            } else {
                const float* src;
                bool f64 = false;
                const double* src64 = nullptr;
                if (i < b1) {          // the parking target area (listed with the areas)
                    src64 = pv.target_xy + 8 * (size_t)e; f64 = true; src = nullptr;
                    cls = T2D_CAMERA_CLASS_TARGET; listing = 0u << 20;
                } else if (i < b2) {   // static obstacle rings
                    const int q = i - b1;
                    cls = T2D_CAMERA_CLASS_OBSTACLE; listing = 0u << 20 | (uint32_t)(1 + q);
                    if (scene) {
                        src = cv.scene_quads + ((size_t)e * T2D_GEN_MAX_QUADS + q) * 8;
                        if (cv.scene_quad_id[(size_t)e * T2D_GEN_MAX_QUADS + q] < 0) n = 0;
                    } else {
                        const int v0 = cv.poly_vert_off[0][s0 + q];
                        n = cv.poly_vert_off[0][s0 + q + 1] - v0;
                        src = cv.poly_xy[0] + 2 * (size_t)v0;
                    }
                } else if (i < b3) {   // lane rings
                    const int q = i - b2;
                    cls = T2D_CAMERA_CLASS_LANE; listing = 1u << 20 | (uint32_t)q;
                    const int v0 = cv.poly_vert_off[1][l0 + q];
                    n = cv.poly_vert_off[1][l0 + q + 1] - v0;
                    src = cv.poly_xy[1] + 2 * (size_t)v0;
                } else {               // track tiles (lanes of the racing map)
                    const int q = i - b3;
                    cls = T2D_CAMERA_CLASS_LANE; listing = 2u << 20 | (uint32_t)q;
                    src = tv.tiles + 8 * (size_t)(t0 + q);
                }
                n = n > kMaxVerts ? kMaxVerts : n;   // (the library admits rings of 3 .. T2D_MAX_POLY_VERTS vertices: never taken)
                float ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
#pragma unroll
                for (int k = 0; k < kMaxVerts; ++k) {
                    if (k >= n) break;
                    const float x = f64 ? (float)src64[2 * k] : src[2 * k], y = f64 ? (float)src64[2 * k + 1] : src[2 * k + 1];
                    r.v[2 * k] = x; r.v[2 * k + 1] = y;
                    const float dx = x - sx, dy = y - sy;
                    const float ux = dx * cyaw - dy * syaw, uy = dx * syaw + dy * cyaw;
                    ulo = fminf(ulo, ux); uhi = fmaxf(uhi, ux); vlo = fminf(vlo, uy); vhi = fmaxf(vhi, uy);
                }
                hit = n >= 3 && (NAIVE || (uhi >= rx0 && ulo <= rx1 && vhi >= ry0 && vlo <= ry1));
            }
            r.key = (uint32_t)cv.z_of_class[cls] << 24 | listing;
            r.kind_n = (uint32_t)kind | (uint32_t)n << 8 | (uint32_t)cls << 16 | (arrow ? 1u << 24 : 0u);
        }
        // append: one ballot and one LDS atomic per wave
        const unsigned long long hits = __ballot(hit);
        int wave_base = 0;
        if (lane == 0 && hits != 0ull) wave_base = atomicAdd(&s_count, __builtin_popcountll(hits));
        wave_base = __shfl(wave_base, 0);
        if (hit) s_rec[wave_base + __builtin_popcountll(hits & ((1ull << lane) - 1ull))] = r;
        __syncthreads();
        // ---- phase 2: four pixels against the list ---------------------------------------------------------------------
        const int count = s_count;
        const uint32_t arrow_z = (uint32_t)cv.z_of_class[T2D_CAMERA_CLASS_HEADING_ARROW] << 24;
        for (int j = 0; j < count; ++j) {
            const Rec& q = s_rec[j];
            const uint32_t key = q.key, kn = q.kind_n;
            const int kind = kn & 0xff, n = (kn >> 8) & 0xff;
            const uint32_t cls_j = (kn >> 16) & 0xff;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (key > best_key[k] && rec_contains(q, kind, n, wx[k], wy[k])) { best_key[k] = key; best_cls[k] = cls_j; }
            if (kn >> 24) {   // the heading triangle of this body: listed right behind it (camera.py:289-301)
                const uint32_t akey = arrow_z | ((key & 0xffffffu) + 1u);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (akey > best_key[k] && rec_contains(q, kTriangle, 0, wx[k], wy[k])) { best_key[k] = akey; best_cls[k] = T2D_CAMERA_CLASS_HEADING_ARROW; }
            }
        }
        __syncthreads();
    }

    // ---- stores -----------------------------------------------------------------------------------------------------------
    if (row >= H || col >= W) return;
    const size_t pix = ((size_t)e * H + row) * W + col;
    if ((W & 3) == 0) {   // (col is a multiple of four: all four pixels are inside, and both addresses are dword-aligned)
        if (out_class) *reinterpret_cast<uint32_t*>(out_class + pix) = best_cls[0] | best_cls[1] << 8 | best_cls[2] << 16 | best_cls[3] << 24;
        if (out_rgb) {
            const uint32_t c0 = cv.palette[best_cls[0]], c1 = cv.palette[best_cls[1]], c2 = cv.palette[best_cls[2]], c3 = cv.palette[best_cls[3]];
            // palette words are r | g << 8 | b << 16: twelve bytes r g b r g b ...
            uint32_t* o = reinterpret_cast<uint32_t*>(out_rgb + 3 * pix);
            o[0] = c0 | c1 << 24;
            o[1] = c1 >> 8 | c2 << 16;
            o[2] = c2 >> 16 | c3 << 8;
        }
    } else {
        for (int k = 0; k < 4 && col + k < W; ++k) {
            if (out_class) out_class[pix + k] = (uint8_t)best_cls[k];
            if (out_rgb) {
                const uint32_t c = cv.palette[best_cls[k]];
                out_rgb[3 * (pix + k)] = (uint8_t)c; out_rgb[3 * (pix + k) + 1] = (uint8_t)(c >> 8); out_rgb[3 * (pix + k) + 2] = (uint8_t)(c >> 16);
            }
        }
    }
}

}  // namespace

hipError_t launch_camera(const PoolView& v, const CameraView& cv, const TrackView& tv, uint8_t* out_class, uint8_t* out_rgb, int naive,
                         hipStream_t s) {
    const int nbx = (cv.width + kBW - 1) / kBW, nby = (cv.height + kBH - 1) / kBH;
    const dim3 grid((unsigned)(nbx * nby) * (unsigned)v.n_env);   // (t2d_camera_config bounds the product)
    if (naive) hipLaunchKernelGGL(camera_kernel<true>, grid, dim3(kBlock), 0, s, v, cv, tv, out_class, out_rgb);
    else hipLaunchKernelGGL(camera_kernel<false>, grid, dim3(kBlock), 0, s, v, cv, tv, out_class, out_rgb);
    return hipGetLastError();
}

}  // namespace t2d
