// Mesh overlay renderer for gfx950 (libairpose_grad.so): what the reference's utils/renderer.py Renderer draws with pyrender -- n posed
// meshes over n background images -- as ray casting on the device.  The contract is in include/airpose_grad.h; the sequence below is
// what tests/render_util.py emulates and counts its error bars from.
//
//   render_prepare_kernel   one thread per max(pixel, vertex): z-buffer entry = EMPTY, camera point p = R v + t, large-face counter = 0
//   render_normal_kernel    one thread per (image, vertex): the sum of its faces' (p1 - p0) x (p2 - p0) in ascending face order through
//                           the vertex -> face CSR table (a gather, no float atomics), normalised
//   render_small_kernel     one thread per (image, face): planes, culling, pixel box.  A box of at most CAP x CAP pixels is walked by
//                           the thread itself: each hit is one 64-bit atomic minimum of (float bits of z) << 32 | face into the
//                           z-buffer.  A larger box (a vertex at z <= znear gives the whole viewport) appends the face to the image's
//                           large list instead, so no thread's work grows with a triangle's screen area.
//   render_large_kernel     one workgroup per 16 x 16 pixel tile and image, one pixel per thread: the image's large list (face and
//                           box) is read 256 entries at a time, the faces whose box meets the tile are set up into LDS and every
//                           thread tests its own pixel against them; the thread's minimum stays in a register and goes to the
//                           z-buffer with one atomic minimum.
//   render_resolve_kernel   one thread per pixel: the winner's planes and w_k are computed again by the SAME functions (face_setup,
//                           ray, edge_w), so the barycentrics are those of the test that was won; shading; rgb, depth, face.
//
// Per face (p0, p1, p2) and pixel (i, j), with `#pragma clang fp contract(off)` so that only the fmaf calls below are fused:
//   cross(a, b) = (fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x)))
//   n0 = cross(p1, p2 - p1), n1 = cross(p2, p0 - p2), n2 = cross(p0, p1 - p0)   (a x (b - a) = a x b: the edge form keeps the
//   rounded products at the size of an edge instead of two camera distances); m = cross(p1 - p0, p2 - p0),
//   det = fmaf(p0.x, m.x, fmaf(p0.y, m.y, p0.z * m.z))   (p0 . m = p0 . (p1 x p2))
//   dx = (((float)j + 0.5f) - cx) / fx, dy = (((float)i + 0.5f) - cy) / fy
//   w_k = fmaf(dx, nk.x, fmaf(dy, nk.y, nk.z)); s = (w0 + w1) + w2; z = det / s
//   drawn iff det < 0, every vertex finite; hit iff w0 <= 0, w1 <= 0, w2 <= 0 and znear <= z <= zfar (s = 0 gives a z that fails)
//   p = v (R NULL) or p_i = fmaf(R_i2, v2, fmaf(R_i1, v1, R_i0 * v0)); then p_i + t_i unless t is NULL
// Shading: N_v = sum of cross(p1 - p0, p2 - p0) over the vertex's faces with finite vertices, n_v = N_v / sqrtf(|N_v|^2) (zero stays zero); b_k = w_k / s;
//   m = fmaf(b2, n_2, fmaf(b1, n_1, b0 * n_0)) per component, l2 = fmaf(m.z, m.z, fmaf(m.y, m.y, m.x * m.x)),
//   c = l2 > 0 ? fmaxf(0, -(m.z / sqrtf(l2))) : 0, shade = fmaf(diffuse, c, ambient), colour = fminf(1, base * shade)
//
// Determinism.  z > 0, so its float bits order like z and the 64-bit minimum is (nearest z, then lowest face) whatever the arrival
// order; the large list's order varies from run to run but only feeds that minimum.  Everything else is plain vector stores.
// Bounds.  No index is formed from an unchecked float (box_lo / box_hi: a NaN gives an empty box); face and CSR entries outside
// their tables are skipped on the device as well, so a bad table draws less and never reads out of bounds.
#include "grad_internal.h"

#include <cmath>
#include <string>

#pragma clang fp contract(off)

namespace {

constexpr int RT = 256;                                  // threads per workgroup
constexpr int CAP = 16;                                  // widest box (pixels, each way) a single thread walks
constexpr int TILE = 16;                                 // render_large_kernel: TILE x TILE pixels per workgroup (= RT)
constexpr unsigned long long EMPTY = ~0ull;
constexpr int MAX_RES = 16384, MAX_N = 65535, MAX_VF = 1 << 24;
constexpr int64_t MAX_ITEMS = (int64_t)1 << 36;            // pixels, vertices or faces over all images: the launches stay below 2^31 workgroups

struct RenderArgs {
    int n, V, F, H, W, csr_len;
    const float* verts;
    const int *faces, *csr_off, *csr_face;
    const float *R, *t;
    float fx, fy, cx, cy, znear, zfar;
    const float* bg;
    float base[3], ambient, diffuse;
    float *rgb, *depth;
    int* face;
    float *pc, *nrm;                                     // workspace: camera points and unit vertex normals, (n, V, 3) each
    unsigned long long* zbuf;                            // (n, H, W)
    int4* list;                                          // (n, F) large faces: face, j0 | j1 << 16, i0 | i1 << 16, unused
    int* count;                                          // (n) how many
};

struct V3 {
    float x, y, z;
};
struct Face {
    V3 n0, n1, n2;
    float det;
    int j0, j1, i0, i1;                                  // the pixel box, inclusive; j0 > j1 or i0 > i1: empty
};

__device__ __forceinline__ V3 cross(const V3& a, const V3& b) {
    return {fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x))};
}
__device__ __forceinline__ V3 sub(const V3& a, const V3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ bool finite3(const V3& a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
__device__ __forceinline__ V3 load3(const float* p) { return {p[0], p[1], p[2]}; }

// first / last index of 0 .. n - 1 at or after / before the (already floored) float f; a NaN gives n / -1, an empty range
__device__ __forceinline__ int box_lo(float f, int n) {
    int r = n;
    if (f < (float)n) r = f > 0.f ? (int)f : 0;
    return r;
}
__device__ __forceinline__ int box_hi(float f, int n) {
    int r = -1;
    if (f >= 0.f) r = f < (float)(n - 1) ? (int)f : n - 1;
    return r;
}

__device__ __forceinline__ float ray(int j, float c, float f) { return (((float)j + 0.5f) - c) / f; }
__device__ __forceinline__ float edge_w(float dx, float dy, const V3& n) { return fmaf(dx, n.x, fmaf(dy, n.y, n.z)); }

// the three vertex indices of face f, or false when one lies outside the vertex table
__device__ __forceinline__ bool face_indices(const RenderArgs& a, int f, int* v) {
    const int* q = a.faces + (size_t)f * 3;
    v[0] = q[0], v[1] = q[1], v[2] = q[2];
    return (unsigned)v[0] < (unsigned)a.V && (unsigned)v[1] < (unsigned)a.V && (unsigned)v[2] < (unsigned)a.V;
}

// planes and determinant of face f of image img; false when the face is not drawn.  The box only with want_box.
__device__ __forceinline__ bool face_setup(const RenderArgs& a, int img, int f, bool want_box, Face& o) {
    int v[3];
    if (!face_indices(a, f, v)) return false;
    const float* pc = a.pc + (size_t)img * a.V * 3;
    const V3 p0 = load3(pc + (size_t)v[0] * 3), p1 = load3(pc + (size_t)v[1] * 3), p2 = load3(pc + (size_t)v[2] * 3);
    if (!(finite3(p0) && finite3(p1) && finite3(p2))) return false;
    // a x b as a x (b - a) and p0 . (p1 x p2) as p0 . ((p1 - p0) x (p2 - p0)): equal in exact arithmetic, and the products that
    // are rounded are of the size of an edge, not of two camera distances
    o.n0 = cross(p1, sub(p2, p1)), o.n1 = cross(p2, sub(p0, p2)), o.n2 = cross(p0, sub(p1, p0));
    const V3 m = cross(sub(p1, p0), sub(p2, p0));
    o.det = fmaf(p0.x, m.x, fmaf(p0.y, m.y, p0.z * m.z));
    if (!(o.det < 0.f)) return false;
    if (!want_box) return true;
    const float zmin = fminf(p0.z, fminf(p1.z, p2.z));
    if (!(zmin > a.znear)) {                             // a vertex at or behind the near plane: the projection bounds nothing
        o.j0 = 0, o.j1 = a.W - 1, o.i0 = 0, o.i1 = a.H - 1;
        return true;
    }
    // pixel j's centre is at j + 0.5, so the pixels to test are ceil(umin - 0.5) .. floor(umax - 0.5); floor(umin - 0.5) ..
    // floor(umax + 0.5) holds them with up to one pixel to spare each way, which covers the roundings here (below 0.01 pixel)
    const float u0 = fmaf(a.fx, p0.x / p0.z, a.cx), u1 = fmaf(a.fx, p1.x / p1.z, a.cx), u2 = fmaf(a.fx, p2.x / p2.z, a.cx);
    const float r0 = fmaf(a.fy, p0.y / p0.z, a.cy), r1 = fmaf(a.fy, p1.y / p1.z, a.cy), r2 = fmaf(a.fy, p2.y / p2.z, a.cy);
    o.j0 = box_lo(floorf(fminf(u0, fminf(u1, u2)) - 0.5f), a.W);
    o.j1 = box_hi(floorf(fmaxf(u0, fmaxf(u1, u2)) + 0.5f), a.W);
    o.i0 = box_lo(floorf(fminf(r0, fminf(r1, r2)) - 0.5f), a.H);
    o.i1 = box_hi(floorf(fmaxf(r0, fmaxf(r1, r2)) + 0.5f), a.H);
    return true;
}

// the hit test of one pixel ray against one face; z is written when it hits
__device__ __forceinline__ bool face_hit(const RenderArgs& a, const V3& n0, const V3& n1, const V3& n2, float det, float dx, float dy,
                                         float& z) {
    const float w0 = edge_w(dx, dy, n0), w1 = edge_w(dx, dy, n1), w2 = edge_w(dx, dy, n2);
    if (!(w0 <= 0.f && w1 <= 0.f && w2 <= 0.f)) return false;
    const float s = (w0 + w1) + w2;
    z = det / s;
    return z >= a.znear && z <= a.zfar;
}

__device__ __forceinline__ unsigned long long pack_key(float z, int f) {
    return ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(unsigned)f;
}

__global__ void __launch_bounds__(RT) render_prepare_kernel(const RenderArgs a) {
    const size_t idx = (size_t)blockIdx.x * RT + threadIdx.x;
    const size_t npix = (size_t)a.n * a.H * a.W, nv = (size_t)a.n * a.V;
    if (idx < npix) a.zbuf[idx] = EMPTY;
    if (idx < (size_t)a.n) a.count[idx] = 0;
    if (idx < nv) {
        const size_t img = idx / a.V;
        const V3 v = load3(a.verts + idx * 3);
        V3 p = v;
        if (a.R) {
            const float* R = a.R + img * 9;
            p.x = fmaf(R[2], v.z, fmaf(R[1], v.y, R[0] * v.x));
            p.y = fmaf(R[5], v.z, fmaf(R[4], v.y, R[3] * v.x));
            p.z = fmaf(R[8], v.z, fmaf(R[7], v.y, R[6] * v.x));
        }
        if (a.t) {
            const float* t = a.t + img * 3;
            p.x = p.x + t[0], p.y = p.y + t[1], p.z = p.z + t[2];
        }
        float* o = a.pc + idx * 3;
        o[0] = p.x, o[1] = p.y, o[2] = p.z;
    }
}

__global__ void __launch_bounds__(RT) render_normal_kernel(const RenderArgs a) {
    const size_t idx = (size_t)blockIdx.x * RT + threadIdx.x;
    if (idx >= (size_t)a.n * a.V) return;
    const int img = (int)(idx / a.V), v = (int)(idx - (size_t)img * a.V);
    const float* pc = a.pc + (size_t)img * a.V * 3;
    int b = a.csr_off[v], e = a.csr_off[v + 1];
    b = b < 0 ? 0 : b;
    e = e > a.csr_len ? a.csr_len : e;
    V3 N = {0.f, 0.f, 0.f};
    for (int k = b; k < e; ++k) {                        // ascending face order: the table is built that way
        const int f = a.csr_face[k];
        int q[3];
        if ((unsigned)f >= (unsigned)a.F || !face_indices(a, f, q)) continue;
        const V3 p0 = load3(pc + (size_t)q[0] * 3), p1 = load3(pc + (size_t)q[1] * 3), p2 = load3(pc + (size_t)q[2] * 3);
        if (!(finite3(p0) && finite3(p1) && finite3(p2))) continue;      // a face that is never drawn lends no normal either
        const V3 m = cross(sub(p1, p0), sub(p2, p0));
        N.x = N.x + m.x, N.y = N.y + m.y, N.z = N.z + m.z;
    }
    const float l2 = fmaf(N.z, N.z, fmaf(N.y, N.y, N.x * N.x));
    if (l2 > 0.f) {
        const float l = sqrtf(l2);
        N.x = N.x / l, N.y = N.y / l, N.z = N.z / l;
    } else {
        N.x = N.y = N.z = 0.f;                           // (also a sum that overflowed)
    }
    float* o = a.nrm + idx * 3;
    o[0] = N.x, o[1] = N.y, o[2] = N.z;
}

__global__ void __launch_bounds__(RT) render_small_kernel(const RenderArgs a) {
    const size_t idx = (size_t)blockIdx.x * RT + threadIdx.x;
    if (idx >= (size_t)a.n * a.F) return;
    const int img = (int)(idx / a.F), f = (int)(idx - (size_t)img * a.F);
    Face fc;
    if (!face_setup(a, img, f, true, fc)) return;
    if (fc.j0 > fc.j1 || fc.i0 > fc.i1) return;
    if (fc.j1 - fc.j0 >= CAP || fc.i1 - fc.i0 >= CAP) {
        const int slot = atomicAdd(a.count + img, 1);    // slot < F: a face is appended at most once per image
        a.list[(size_t)img * a.F + slot] = make_int4(f, fc.j0 | (fc.j1 << 16), fc.i0 | (fc.i1 << 16), 0);   // each below 2^14
        return;
    }
    unsigned long long* zb = a.zbuf + (size_t)img * a.H * a.W;
    for (int i = fc.i0; i <= fc.i1; ++i) {
        const float dy = ray(i, a.cy, a.fy);
        for (int j = fc.j0; j <= fc.j1; ++j) {
            float z;
            if (face_hit(a, fc.n0, fc.n1, fc.n2, fc.det, ray(j, a.cx, a.fx), dy, z)) atomicMin(zb + (size_t)i * a.W + j, pack_key(z, f));
        }
    }
}

__global__ void __launch_bounds__(RT) render_large_kernel(const RenderArgs a) {
    __shared__ Face sf[RT];
    __shared__ int sid[RT];                              // the face's index, -1: not drawn
    const int img = blockIdx.y;
    const int tiles_x = (a.W + TILE - 1) / TILE;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int tj0 = tx * TILE, ti0 = ty * TILE;
    const int tj1 = tj0 + TILE - 1, ti1 = ti0 + TILE - 1;
    const int j = tj0 + (threadIdx.x & (TILE - 1)), i = ti0 + (threadIdx.x >> 4);
    const bool inside = i < a.H && j < a.W;
    const float dx = ray(j, a.cx, a.fx), dy = ray(i, a.cy, a.fy);
    int cnt = a.count[img];
    cnt = cnt > a.F ? a.F : cnt;
    unsigned long long best = EMPTY;
    for (int c0 = 0; c0 < cnt; c0 += RT) {
        const int k = c0 + threadIdx.x;
        int id = -1;
        if (k < cnt) {                                   // set up only the faces whose box meets this tile
            const int4 e = a.list[(size_t)img * a.F + k];
            const int j0 = e.y & 0xffff, j1 = (e.y >> 16) & 0xffff, i0 = e.z & 0xffff, i1 = (e.z >> 16) & 0xffff;
            if (!(j0 > tj1 || j1 < tj0 || i0 > ti1 || i1 < ti0) && (unsigned)e.x < (unsigned)a.F &&
                face_setup(a, img, e.x, false, sf[threadIdx.x])) {
                Face& o = sf[threadIdx.x];
                o.j0 = j0, o.j1 = j1, o.i0 = i0, o.i1 = i1;
                id = e.x;
            }
        }
        sid[threadIdx.x] = id;
        __syncthreads();
        const int m = cnt - c0 < RT ? cnt - c0 : RT;
        for (int q = 0; q < m; ++q) {
            const int f = sid[q];
            if (f < 0) continue;
            const Face& fc = sf[q];
            if (j < fc.j0 || j > fc.j1 || i < fc.i0 || i > fc.i1) continue;
            float z;
            if (face_hit(a, fc.n0, fc.n1, fc.n2, fc.det, dx, dy, z)) {
                const unsigned long long key = pack_key(z, f);
                best = key < best ? key : best;
            }
        }
        __syncthreads();
    }
    if (inside && best != EMPTY) atomicMin(a.zbuf + ((size_t)img * a.H + i) * a.W + j, best);
}

__global__ void __launch_bounds__(RT) render_resolve_kernel(const RenderArgs a) {
    const size_t idx = (size_t)blockIdx.x * RT + threadIdx.x;
    const size_t hw = (size_t)a.H * a.W;
    if (idx >= (size_t)a.n * hw) return;
    const int img = (int)(idx / hw);
    const size_t pix = idx - (size_t)img * hw;
    const int i = (int)(pix / a.W), j = (int)(pix - (size_t)i * a.W);
    const size_t c0 = (size_t)img * 3 * hw + pix;
    const unsigned long long key = a.zbuf[idx];
    const int f = (int)(unsigned)(key & 0xffffffffull);
    Face fc;
    if (key == EMPTY || (unsigned)f >= (unsigned)a.F || !face_setup(a, img, f, false, fc)) {
        a.rgb[c0] = a.bg ? a.bg[c0] : 0.f;
        a.rgb[c0 + hw] = a.bg ? a.bg[c0 + hw] : 0.f;
        a.rgb[c0 + 2 * hw] = a.bg ? a.bg[c0 + 2 * hw] : 0.f;
        if (a.depth) a.depth[idx] = 0.f;
        if (a.face) a.face[idx] = -1;
        return;
    }
    const float dx = ray(j, a.cx, a.fx), dy = ray(i, a.cy, a.fy);
    const float w0 = edge_w(dx, dy, fc.n0), w1 = edge_w(dx, dy, fc.n1), w2 = edge_w(dx, dy, fc.n2);
    const float s = (w0 + w1) + w2;
    const float b0 = w0 / s, b1 = w1 / s, b2 = w2 / s;
    int v[3];
    face_indices(a, f, v);                               // in range: face_setup has checked them
    const float* nr = a.nrm + (size_t)img * a.V * 3;
    const V3 m0 = load3(nr + (size_t)v[0] * 3), m1 = load3(nr + (size_t)v[1] * 3), m2 = load3(nr + (size_t)v[2] * 3);
    const float mx = fmaf(b2, m2.x, fmaf(b1, m1.x, b0 * m0.x));
    const float my = fmaf(b2, m2.y, fmaf(b1, m1.y, b0 * m0.y));
    const float mz = fmaf(b2, m2.z, fmaf(b1, m1.z, b0 * m0.z));
    const float l2 = fmaf(mz, mz, fmaf(my, my, mx * mx));
    float c = 0.f;
    if (l2 > 0.f) c = fmaxf(0.f, -(mz / sqrtf(l2)));
    const float shade = fmaf(a.diffuse, c, a.ambient);
    a.rgb[c0] = fminf(1.f, a.base[0] * shade);
    a.rgb[c0 + hw] = fminf(1.f, a.base[1] * shade);
    a.rgb[c0 + 2 * hw] = fminf(1.f, a.base[2] * shade);
    if (a.depth) a.depth[idx] = __uint_as_float((unsigned)(key >> 32));
    if (a.face) a.face[idx] = f;
}

inline int64_t al256(int64_t b) { return (b + 255) & ~(int64_t)255; }

struct Layout {
    int64_t pc, nrm, zbuf, list, count, total;
};

inline bool sizes_ok(int n, int H, int W, int V, int F) {
    if (!(n >= 0 && n <= MAX_N && H >= 1 && H <= MAX_RES && W >= 1 && W <= MAX_RES && V >= 1 && V <= MAX_VF && F >= 1 && F <= MAX_VF))
        return false;
    return (int64_t)n * H * W <= MAX_ITEMS && (int64_t)n * V <= MAX_ITEMS && (int64_t)n * F <= MAX_ITEMS;
}

inline Layout layout(int n, int H, int W, int V, int F) {
    const int64_t m = n > 0 ? n : 1;
    Layout l;
    l.pc = 0;
    l.nrm = l.pc + al256(m * V * 3 * 4);
    l.zbuf = l.nrm + al256(m * V * 3 * 4);
    l.list = l.zbuf + al256(m * H * W * 8);
    l.count = l.list + al256(m * F * 16);
    l.total = l.count + al256(m * 4);
    return l;
}

}  // namespace

extern "C" {

int64_t apg_render_workspace_bytes(int n, int H, int W, int V, int F) {
    if (!sizes_ok(n, H, W, V, F)) return -1;
    return layout(n, H, W, V, F).total;
}

int apg_render_overlay(int n, int V, int F, int H, int W, const float* vertices, const int* faces, const int* csr_offsets,
                       const int* csr_faces, int csr_len, const float* R, const float* t, float fx, float fy, float cx, float cy,
                       float znear, float zfar, const float* background, float base_r, float base_g, float base_b, float ambient,
                       float diffuse, float* out_rgb, float* out_depth, int* out_face, void* workspace, int64_t workspace_bytes,
                       void* stream) {
    const std::string f = "apg_render_overlay: ";
    if (n < 0 || n > MAX_N) return apg_fail(APG_EINVAL, f + "n must be in 0 .. " + std::to_string(MAX_N));
    if (V < 1 || V > MAX_VF) return apg_fail(APG_EINVAL, f + "V must be in 1 .. " + std::to_string(MAX_VF));
    if (F < 1 || F > MAX_VF) return apg_fail(APG_EINVAL, f + "F must be in 1 .. " + std::to_string(MAX_VF));
    if (H < 1 || H > MAX_RES) return apg_fail(APG_EINVAL, f + "H must be in 1 .. " + std::to_string(MAX_RES));
    if (W < 1 || W > MAX_RES) return apg_fail(APG_EINVAL, f + "W must be in 1 .. " + std::to_string(MAX_RES));
    if (!sizes_ok(n, H, W, V, F)) return apg_fail(APG_EINVAL, f + "n times H W, V or F must not exceed 2^36");
    if (csr_len < 0 || (int64_t)csr_len > (int64_t)3 * F) return apg_fail(APG_EINVAL, f + "csr_len must be in 0 .. 3 F");
    if (!vertices) return apg_fail(APG_EINVAL, f + "vertices is NULL");
    if (!faces) return apg_fail(APG_EINVAL, f + "faces is NULL");
    if (!csr_offsets) return apg_fail(APG_EINVAL, f + "csr_offsets is NULL");
    if (!csr_faces) return apg_fail(APG_EINVAL, f + "csr_faces is NULL");
    if (!out_rgb) return apg_fail(APG_EINVAL, f + "out_rgb is NULL");
    if (!workspace) return apg_fail(APG_EINVAL, f + "workspace is NULL");
    if (!(fx > 0.f) || !std::isfinite(fx)) return apg_fail(APG_EINVAL, f + "fx must be positive and finite");
    if (!(fy > 0.f) || !std::isfinite(fy)) return apg_fail(APG_EINVAL, f + "fy must be positive and finite");
    if (!std::isfinite(cx)) return apg_fail(APG_EINVAL, f + "cx must be finite");
    if (!std::isfinite(cy)) return apg_fail(APG_EINVAL, f + "cy must be finite");
    if (!(znear > 0.f) || !std::isfinite(znear)) return apg_fail(APG_EINVAL, f + "znear must be positive and finite");
    if (!(zfar >= znear) || !std::isfinite(zfar)) return apg_fail(APG_EINVAL, f + "zfar must be finite and at least znear");
    const float shading[5] = {base_r, base_g, base_b, ambient, diffuse};
    static const char* const sname[5] = {"base_r", "base_g", "base_b", "ambient", "diffuse"};
    for (int k = 0; k < 5; ++k)
        if (!(shading[k] >= 0.f) || !std::isfinite(shading[k])) return apg_fail(APG_EINVAL, f + sname[k] + " must be finite and not negative");
    const void* p4[10] = {vertices, faces, csr_offsets, csr_faces, R, t, background, out_rgb, out_depth, out_face};
    static const char* const n4[10] = {"vertices", "faces", "csr_offsets", "csr_faces", "R", "t", "background", "out_rgb", "out_depth", "out_face"};
    for (int k = 0; k < 10; ++k)
        if ((uintptr_t)p4[k] & 3) return apg_fail(APG_EINVAL, f + n4[k] + " is not 4-byte aligned");
    if ((uintptr_t)workspace & 15) return apg_fail(APG_EINVAL, f + "workspace is not 16-byte aligned");
    if (background && (const void*)background == (const void*)out_rgb) return apg_fail(APG_EINVAL, f + "out_rgb must not be the background");
    const Layout l = layout(n, H, W, V, F);
    if (workspace_bytes < l.total)
        return apg_fail(APG_ENOMEM, f + "workspace of " + std::to_string(workspace_bytes) + " bytes, apg_render_workspace_bytes asks for " +
                                        std::to_string(l.total));
    if (n == 0) return APG_OK;                            // nothing to draw: no launch

    RenderArgs a = {};
    a.n = n, a.V = V, a.F = F, a.H = H, a.W = W, a.csr_len = csr_len;
    a.verts = vertices, a.faces = faces, a.csr_off = csr_offsets, a.csr_face = csr_faces, a.R = R, a.t = t;
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy, a.znear = znear, a.zfar = zfar;
    a.bg = background;
    a.base[0] = base_r, a.base[1] = base_g, a.base[2] = base_b, a.ambient = ambient, a.diffuse = diffuse;
    a.rgb = out_rgb, a.depth = out_depth, a.face = out_face;
    char* ws = (char*)workspace;
    a.pc = (float*)(ws + l.pc), a.nrm = (float*)(ws + l.nrm), a.zbuf = (unsigned long long*)(ws + l.zbuf);
    a.list = (int4*)(ws + l.list), a.count = (int*)(ws + l.count);

    const int64_t npix = (int64_t)n * H * W, nv = (int64_t)n * V, nf = (int64_t)n * F;
    const auto blocks = [](int64_t items) { return dim3((unsigned)((items + RT - 1) / RT)); };
    const int tiles = ((W + TILE - 1) / TILE) * ((H + TILE - 1) / TILE);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(render_prepare_kernel, blocks(npix > nv ? npix : nv), dim3(RT), 0, st, a);
    APG_TRY(hipGetLastError());
    hipLaunchKernelGGL(render_normal_kernel, blocks(nv), dim3(RT), 0, st, a);
    APG_TRY(hipGetLastError());
    hipLaunchKernelGGL(render_small_kernel, blocks(nf), dim3(RT), 0, st, a);
    APG_TRY(hipGetLastError());
    hipLaunchKernelGGL(render_large_kernel, dim3((unsigned)tiles, (unsigned)n), dim3(RT), 0, st, a);
    APG_TRY(hipGetLastError());
    hipLaunchKernelGGL(render_resolve_kernel, blocks(npix), dim3(RT), 0, st, a);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

}  // extern "C"
