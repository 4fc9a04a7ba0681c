// Camera roll (libairpose_grad.so): a rotation of the camera about its optical axis, applied to the crops AND to every label of a
// SyntheticBatches / RealSequenceBatches dict.  The contract -- the geometry, the order of every fp32 operation, the refusal, the
// status bits, the draw -- is in include/airpose_grad.h ("Camera roll (roll.hip)").  The reference has no image-plane augmentation:
// its rottrans_tfm (dsets/aerialpeople.py, not called) moves the WORLD frame -- extr and the *_wrt_origin labels -- and no pixel.
//
//   roll_draw_kernel     grid = ceil(2 n / 64): one thread per (suffix, sample) writes (cos, sin); cos and sin of the fp32 angle are
//     taken in fp64 and rounded once, the only transcendental calls of this file.
//   roll_labels_kernel   grid = (ceil(items / 256), n, 2 suffixes): a streaming kernel, one thread per item -- a vertex, a joint, a
//     2-D point, a column of orient or of extr, trans -- each read once and written once (12-byte items, consecutive lanes on
//     consecutive items).  Every thread re-derives the (sample, view)'s decision from rot, intr and bb (five cached loads and a dozen
//     flops: cheaper than a second launch or a barrier); thread 0 of block 0 writes rot_used, bb' and status with plain stores.
//   roll_crops_kernel    grid = (196 tiles of 16 x 16 pixels, n, 2 suffixes), 256 threads: a gather kernel, one thread per output
//     pixel and all three channels, like preprocess_kernel.  A (1, 0) row IS preprocess_px; a rolled row turns preprocess_px's own pre-floor source
//     position about the box centre and samples the zero-continued canvas bilinearly, every tap bounds-checked.
// Compiled with -ffp-contract=off -fno-slp-vectorize (csrc/Makefile): every operation outside the draw is a single fp32 (or, for
// the source position, fp64) rounding in the written order, and there is no packed fp32 math.  No atomic, no LDS, plain vector
// stores only.
#include "grad_internal.h"

#include <cmath>
#include <string>

namespace {

constexpr int IMG = 224, NT = APG_ROLL_THREADS;
static_assert(NT == 16 * 16 && IMG % 16 == 0, "roll_crops_kernel: a 16 x 16 tile per workgroup");
constexpr int MAX_N = 65535, MAX_V = 1 << 24, MAX_J = 1 << 16, MAX_SIDE = 1 << 20;

struct LabelArgs {
    int n, V, J, P, ps, cam_all;
    int Hc[2], Wc[2];
    const int *cam, *crops;
    const float *rot, *intr, *bb;
    const float *verts, *joints, *orient, *trans, *extr, *j2d, *j2dc;
    float *rot_used, *bb_out;
    int* status;
    float *verts_o, *joints_o, *orient_o, *trans_o, *extr_o, *j2d_o, *j2dc_o;
};

struct CropArgs {
    int n, bgr, cam_all;
    int Hc[2], Wc[2];
    const unsigned char* frames[2];
    const int *cam, *crops;
    const float *intr, *rot_used;
    float* im;
};

#include "draws.inc"
#include "preprocess_px.inc"

// what a (sample, view) turns by: (c, sn), tx = sn fx / fy, ty = sn fy / fx, the principal point
struct Turn {
    float c, sn, tx, ty, cx, cy;
    bool ident;
};

__device__ __forceinline__ Turn turn_of(float c, float sn, const float* __restrict__ K) {
    Turn t;
    t.c = c; t.sn = sn; t.cx = K[2]; t.cy = K[5];
    const float kx = K[0] / K[4], ky = K[4] / K[0];
    t.ident = c == 1.f && sn == 0.f;
    t.tx = t.ident ? 0.f : sn * kx;                          // (exactly 0 on an un-rolled row, whatever intr holds)
    t.ty = t.ident ? 0.f : sn * ky;
    return t;
}

// A(theta) (x, y)
__device__ __forceinline__ void fwd(const Turn& t, float x, float y, float& xo, float& yo) {
    xo = (t.c * x) - (t.tx * y);
    yo = (t.ty * x) + (t.c * y);
}
// A(-theta) (x, y)
__device__ __forceinline__ void back(const Turn& t, float x, float y, float& xo, float& yo) {
    xo = (t.c * x) + (t.tx * y);
    yo = (t.c * y) - (t.ty * x);
}
// Rz(theta) (x, y): the camera-frame labels
__device__ __forceinline__ void rz(const Turn& t, float x, float y, float& xo, float& yo) {
    xo = (t.c * x) - (t.sn * y);
    yo = (t.sn * x) + (t.c * y);
}

__global__ void __launch_bounds__(64) roll_draw_kernel(int n, int cam_all, uint32_t k0, uint32_t k1, uint32_t epoch,
                                                       const int* __restrict__ index, const int* __restrict__ cam, float p,
                                                       float max_rad, float* __restrict__ rot) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= 2 * n) return;
    const int s = g / n, i = g - s * n;
    const uint32_t cm = (uint32_t)(((cam ? cam[i] : cam_all) & 1) ^ s);
    const U4 d = philox((uint32_t)index[i], epoch, cm, 15u, k0, k1);
    float c = 1.f, sn = 0.f;
    if (uni(d.w[0]) < p) {
        const float ang = ((2.f * uni(d.w[1])) - 1.f) * max_rad;
        c = (float)cos((double)ang);
        sn = (float)sin((double)ang);
    }
    rot[(size_t)g * 2] = c;
    rot[(size_t)g * 2 + 1] = sn;
}

__global__ void __launch_bounds__(NT) roll_labels_kernel(const LabelArgs a) {
    const int i = blockIdx.y, s = blockIdx.z, n = a.n;
    const size_t f = (size_t)s * n + i;
    // the decision, the same in every thread of the (sample, view)
    Turn t = turn_of(a.rot[f * 2], a.rot[f * 2 + 1], a.intr + f * 9);
    const float bx = a.bb[f * 3], by = a.bb[f * 3 + 1];
    float nbx = bx, nby = by;
    int st = 0;
    if (!t.ident) {
        float u, v;
        fwd(t, bx * t.cx, by * t.cy, u, v);
        nbx = u / t.cx; nby = v / t.cy;
        if (!(fabsf(nbx) <= 1.f && fabsf(nby) <= 1.f)) {     // (a NaN is refused too)
            st |= APG_ROLL_CENTRE_OUT;
            t.c = 1.f; t.sn = 0.f; t.tx = 0.f; t.ty = 0.f; t.ident = true;
            nbx = bx; nby = by;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int cm = ((a.cam ? a.cam[i] : a.cam_all) & 1) ^ s;
        const int* cr = a.crops + f * 4;
        const float hh = (float)((long long)cr[1] - cr[0]) * 0.5f, hw = (float)((long long)cr[3] - cr[2]) * 0.5f;
        const float my = (float)cr[0] + hh, mx = (float)cr[2] + hw, Hf = (float)a.Hc[cm], Wf = (float)a.Wc[cm];
        bool off = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float ux = (k & 1) ? hw : -hw, uy = (k & 2) ? hh : -hh;
            float rx, ry;
            back(t, ux, uy, rx, ry);
            const float qx = mx + rx, qy = my + ry;
            off = off || !(qx >= 0.f && qx <= Wf && qy >= 0.f && qy <= Hf);
        }
        if (off) st |= APG_ROLL_OFF_CANVAS;
        a.rot_used[f * 2] = t.ident ? 1.f : t.c;
        a.rot_used[f * 2 + 1] = t.ident ? 0.f : t.sn;
        a.bb_out[f * 3] = nbx;
        a.bb_out[f * 3 + 1] = nby;
        a.bb_out[f * 3 + 2] = a.bb[f * 3 + 2];
        a.status[f] = st;
    }

    // the thread's item
    int k = blockIdx.x * NT + threadIdx.x;
    const int nv = a.verts ? a.V : 0, nj = a.joints ? a.J : 0, np2 = a.j2d ? a.P : 0, npc = a.j2dc ? a.P : 0;
    if (k < nv + nj) {                                       // a vertex or a joint: Rz (x, y), z copied
        const bool vert = k < nv;
        const size_t at = vert ? (f * a.V + k) * 3 : (f * a.J + (k - nv)) * 3;
        const float* src = (vert ? a.verts : a.joints) + at;
        float* dst = (vert ? a.verts_o : a.joints_o) + at;
        const float x = src[0], y = src[1], z = src[2];
        float xo = x, yo = y;
        if (!t.ident) rz(t, x, y, xo, yo);
        dst[0] = xo; dst[1] = yo; dst[2] = z;
        return;
    }
    k -= nv + nj;
    if (k < np2 + npc) {                                     // a 2-D point: about the principal point, or the vector itself
        const bool frame = k < np2;
        const size_t at = (f * a.P + (frame ? k : k - np2)) * a.ps;
        const float* src = (frame ? a.j2d : a.j2dc) + at;
        float* dst = (frame ? a.j2d_o : a.j2dc_o) + at;
        const float x = src[0], y = src[1];
        float xo = x, yo = y;
        if (!t.ident) {
            if (frame) {
                float u, v;
                fwd(t, x - t.cx, y - t.cy, u, v);
                xo = t.cx + u; yo = t.cy + v;
            } else {
                fwd(t, x, y, xo, yo);
            }
        }
        dst[0] = xo; dst[1] = yo;
        if (a.ps == 3) dst[2] = src[2];
        return;
    }
    k -= np2 + npc;
    if (k == 0) {
        if (a.trans) {
            const float* src = a.trans + f * 3;
            float* dst = a.trans_o + f * 3;
            const float x = src[0], y = src[1], z = src[2];
            float xo = x, yo = y;
            if (!t.ident) rz(t, x, y, xo, yo);
            dst[0] = xo; dst[1] = yo; dst[2] = z;
        }
    } else if (k < 4) {                                      // column k - 1 of orient: rows 0 and 1 mixed, row 2 copied
        if (a.orient) {
            const float* src = a.orient + f * 9 + (k - 1);
            float* dst = a.orient_o + f * 9 + (k - 1);
            const float x = src[0], y = src[3], z = src[6];
            float xo = x, yo = y;
            if (!t.ident) rz(t, x, y, xo, yo);
            dst[0] = xo; dst[3] = yo; dst[6] = z;
        }
    } else if (k < 8) {                                      // column k - 4 of extr: rows 0 and 1 mixed, rows 2 and 3 copied
        if (a.extr) {
            const float* src = a.extr + f * 16 + (k - 4);
            float* dst = a.extr_o + f * 16 + (k - 4);
            const float x = src[0], y = src[4], z = src[8], w = src[12];
            float xo = x, yo = y;
            if (!t.ident) rz(t, x, y, xo, yo);
            dst[0] = xo; dst[4] = yo; dst[8] = z; dst[12] = w;
        }
    }
}

__global__ void __launch_bounds__(NT) roll_crops_kernel(const CropArgs a) {
    // a 16 x 16 tile of output pixels per workgroup, 4 rows x 16 columns per wave: a wave's taps stay within a few canvas rows
    // whatever the angle, where 64 pixels of one output row would cross dozens
    const int i = blockIdx.y, s = blockIdx.z, n = a.n;
    const int px = ((int)(blockIdx.x / (IMG / 16)) * 16 + (int)(threadIdx.x >> 4)) * IMG + (int)(blockIdx.x % (IMG / 16)) * 16 + (int)(threadIdx.x & 15);
    const size_t f = (size_t)s * n + i;
    const int cm = ((a.cam ? a.cam[i] : a.cam_all) & 1) ^ s;
    const int Hc = a.Hc[cm], Wc = a.Wc[cm];
    const int* cr = a.crops + f * 4;
    const int y0 = cr[0], y1 = cr[1], x0 = cr[2], x1 = cr[3];
    if (y0 < 0 || y1 <= y0 || y1 > Hc || x0 < 0 || x1 <= x0 || x1 > Wc) return;           // the whole workgroup
    const unsigned char* fr = a.frames[cm] + (size_t)i * Hc * Wc * 3;
    float* out = a.im + f * 3 * IMG * IMG;
    const Turn t = turn_of(a.rot_used[f * 2], a.rot_used[f * 2 + 1], a.intr + f * 9);
    if (t.ident) {                                           // the batch's own image, bit for bit
        float sc;
        int pd[2];
        preprocess_px(fr, Wc, a.bgr, cr, out, &sc, pd, px);
        return;
    }
    if (px >= IMG * IMG) return;
    // preprocess_px.inc's letter-box and source position, before the floor
    const int h = y1 - y0, w = x1 - x0;
    const double scale = 224.0 / (double)(h > w ? h : w);
    const int dw = (int)(scale * w), dh = (int)(scale * h);
    const int pad_top = (224 - dh) / 2, pad_left = (224 - dw) / 2;
    const int oy = px / 224, ox = px - oy * 224, dy = oy - pad_top, dx = ox - pad_left;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    float v[3] = {0.f, 0.f, 0.f};
    if (dy >= 0 && dy < dh && dx >= 0 && dx < dw) {
        const double sxd = 1.0 / ((double)dw / (double)w), syd = 1.0 / ((double)dh / (double)h);
        const float fx = (float)((dx + 0.5) * sxd - 0.5), fy = (float)((dy + 0.5) * syd - 0.5);
        const float hw = (float)w * 0.5f, hh = (float)h * 0.5f;
        float rx, ry;
        back(t, fx - hw, fy - hh, rx, ry);
        const float qx = ((float)x0 + hw) + rx, qy = ((float)y0 + hh) + ry;
        if (qx > -1.f && qx < (float)Wc && qy > -1.f && qy < (float)Hc) {                  // else no tap lies on the canvas
            const float flx = floorf(qx), fly = floorf(qy);
            const int ix = (int)flx, iy = (int)fly;          // -1 .. Wc - 1, -1 .. Hc - 1
            const float ax = qx - flx, ay = qy - fly;
            const bool l = ix >= 0, r = ix + 1 < Wc, u = iy >= 0, d = iy + 1 < Hc;
            // a tap's offset is formed only where the tap lies on the canvas
            const size_t row = (size_t)Wc * 3;
            const size_t o00 = u && l ? (size_t)iy * row + (size_t)ix * 3 : 0, o01 = u && r ? (size_t)iy * row + (size_t)(ix + 1) * 3 : 0;
            const size_t o10 = d && l ? (size_t)(iy + 1) * row + (size_t)ix * 3 : 0, o11 = d && r ? (size_t)(iy + 1) * row + (size_t)(ix + 1) * 3 : 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int cs = a.bgr ? 2 - c : c;
                const float t00 = u && l ? fr[o00 + cs] / 255.f : 0.f, t01 = u && r ? fr[o01 + cs] / 255.f : 0.f;
                const float t10 = d && l ? fr[o10 + cs] / 255.f : 0.f, t11 = d && r ? fr[o11 + cs] / 255.f : 0.f;
                const float top = (t00 * (1.f - ax)) + (t01 * ax), bot = (t10 * (1.f - ax)) + (t11 * ax);
                v[c] = (top * (1.f - ay)) + (bot * ay);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[((size_t)c * 224 + oy) * 224 + ox] = (v[c] - mean[c]) / stdv[c];
}

int check_n_cam(const std::string& f, int n, const int* cam, int cam_all) {
    if (n < 1 || n > MAX_N) return apg_fail(APG_EINVAL, f + "n must be in 1 .. " + std::to_string(MAX_N));
    if ((uintptr_t)cam & 3u) return apg_fail(APG_EINVAL, f + "cam is not 4-byte aligned");
    if (cam_all != 0 && cam_all != 1) return apg_fail(APG_EINVAL, f + "cam_all must be 0 or 1");
    return APG_OK;
}

int check_canvases(const std::string& f, int Hc0, int Wc0, int Hc1, int Wc1) {
    const struct { int v; const char* name; } sides[] = {{Hc0, "Hc0"}, {Wc0, "Wc0"}, {Hc1, "Hc1"}, {Wc1, "Wc1"}};
    for (const auto& s : sides)
        if (s.v < 1 || s.v > MAX_SIDE) return apg_fail(APG_EINVAL, f + s.name + " must be in 1 .. " + std::to_string(MAX_SIDE));
    return APG_OK;
}

bool overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

}  // namespace

extern "C" int apg_roll_draw(int n, uint64_t seed, int epoch, const int* index, const int* cam, int cam_all, float p, float max_rad,
                             float* rot, void* stream) {
    const std::string f = "apg_roll_draw: ";
    const ApgPtr ps[] = {{index, "index", 4}, {rot, "rot", 4}};
    if (int rc = apg_check_ptrs(f, ps, 2)) return rc;
    if (int rc = check_n_cam(f, n, cam, cam_all)) return rc;
    if (!(p >= 0.f && p <= 1.f)) return apg_fail(APG_EINVAL, f + "p must be in 0 .. 1");
    if (!(max_rad >= 0.f && max_rad <= 3.1415927f)) return apg_fail(APG_EINVAL, f + "max_rad must be in 0 .. pi");
    hipLaunchKernelGGL(roll_draw_kernel, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, n, cam_all,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)epoch, index, cam, p, max_rad, rot);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

extern "C" int apg_roll_labels(int n, int V, int J, int P, int pstride, int Hc0, int Wc0, int Hc1, int Wc1, const int* cam,
                               int cam_all, const float* rot, const float* intr, const float* bb, const int* crops,
                               const float* verts, const float* joints, const float* orient, const float* trans, const float* extr,
                               const float* j2d, const float* j2d_crop, float* rot_used, float* bb_out, int* status, float* verts_out,
                               float* joints_out, float* orient_out, float* trans_out, float* extr_out, float* j2d_out,
                               float* j2d_crop_out, void* stream) {
    const std::string f = "apg_roll_labels: ";
    const ApgPtr ps[] = {{rot, "rot", 4}, {intr, "intr", 4}, {bb, "bb", 4}, {crops, "crops", 4}, {rot_used, "rot_used", 4},
                         {bb_out, "bb_out", 4}, {status, "status", 4}};
    if (int rc = apg_check_ptrs(f, ps, 7)) return rc;
    if (int rc = check_n_cam(f, n, cam, cam_all)) return rc;
    if (int rc = check_canvases(f, Hc0, Wc0, Hc1, Wc1)) return rc;
    const size_t rows = (size_t)2 * n;
    // a label: NULL = the dict has no such key (its output is not looked at); present = its output is needed
    const struct { const float* in; float* out; const char *name, *out_name; size_t per_row; } labels[] = {
        {verts, verts_out, "verts", "verts_out", (size_t)V * 3}, {joints, joints_out, "joints", "joints_out", (size_t)J * 3},
        {orient, orient_out, "orient", "orient_out", 9}, {trans, trans_out, "trans", "trans_out", 3},
        {extr, extr_out, "extr", "extr_out", 16}, {j2d, j2d_out, "j2d", "j2d_out", (size_t)P * pstride},
        {j2d_crop, j2d_crop_out, "j2d_crop", "j2d_crop_out", (size_t)P * pstride}};
    if (verts && (V < 1 || V > MAX_V)) return apg_fail(APG_EINVAL, f + "V must be in 1 .. " + std::to_string(MAX_V));
    if (joints && (J < 1 || J > MAX_J)) return apg_fail(APG_EINVAL, f + "J must be in 1 .. " + std::to_string(MAX_J));
    if (j2d || j2d_crop) {
        if (P < 1 || P > MAX_J) return apg_fail(APG_EINVAL, f + "P must be in 1 .. " + std::to_string(MAX_J));
        if (pstride != 2 && pstride != 3) return apg_fail(APG_EINVAL, f + "pstride must be 2 or 3");
    }
    for (const auto& l : labels) {
        if (!l.in) continue;
        const ApgPtr pair[] = {{l.in, l.name, 4}, {l.out, l.out_name, 4}};
        if (int rc = apg_check_ptrs(f, pair, 2)) return rc;
        if (overlap(l.in, l.out, rows * l.per_row * sizeof(float)))
            return apg_fail(APG_EINVAL, f + l.out_name + " must not overlap " + l.name);
    }
    if (overlap(rot, rot_used, rows * 2 * sizeof(float))) return apg_fail(APG_EINVAL, f + "rot_used must not overlap rot");
    if (overlap(bb, bb_out, rows * 3 * sizeof(float))) return apg_fail(APG_EINVAL, f + "bb_out must not overlap bb");
    const LabelArgs k = {n, V, J, P, pstride, cam_all, {Hc0, Hc1}, {Wc0, Wc1}, cam, crops, rot, intr, bb, verts, joints, orient, trans,
                         extr, j2d, j2d_crop, rot_used, bb_out, status, verts_out, joints_out, orient_out, trans_out, extr_out,
                         j2d_out, j2d_crop_out};
    const long long items = (long long)(verts ? V : 0) + (joints ? J : 0) + (j2d ? P : 0) + (j2d_crop ? P : 0) + 8;
    hipLaunchKernelGGL(roll_labels_kernel, dim3((unsigned)((items + NT - 1) / NT), (unsigned)n, 2), dim3(NT), 0, (hipStream_t)stream, k);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

extern "C" int apg_roll_crops(int n, int Hc0, int Wc0, int Hc1, int Wc1, int bgr, const unsigned char* frames0,
                              const unsigned char* frames1, const int* cam, int cam_all, const int* crops, const float* intr,
                              const float* rot_used, float* im, void* stream) {
    const std::string f = "apg_roll_crops: ";
    if (!frames0) return apg_fail(APG_EINVAL, f + "frames0 is NULL");
    if (!frames1) return apg_fail(APG_EINVAL, f + "frames1 is NULL");
    const ApgPtr ps[] = {{crops, "crops", 4}, {intr, "intr", 4}, {rot_used, "rot_used", 4}, {im, "im", 4}};
    if (int rc = apg_check_ptrs(f, ps, 4)) return rc;
    if (int rc = check_n_cam(f, n, cam, cam_all)) return rc;
    if (int rc = check_canvases(f, Hc0, Wc0, Hc1, Wc1)) return rc;
    if (bgr != 0 && bgr != 1) return apg_fail(APG_EINVAL, f + "bgr must be 0 or 1");
    const size_t im_bytes = (size_t)2 * n * 3 * IMG * IMG * sizeof(float);
    const unsigned char* fr[2] = {frames0, frames1};
    const size_t fr_bytes[2] = {(size_t)n * Hc0 * Wc0 * 3, (size_t)n * Hc1 * Wc1 * 3};
    for (int c = 0; c < 2; ++c) {
        const uintptr_t x = (uintptr_t)im, y = (uintptr_t)fr[c];
        if (x < y + fr_bytes[c] && y < x + im_bytes) return apg_fail(APG_EINVAL, f + "im must not overlap frames" + std::to_string(c));
    }
    const CropArgs k = {n, bgr, cam_all, {Hc0, Hc1}, {Wc0, Wc1}, {frames0, frames1}, cam, crops, intr, rot_used, im};
    hipLaunchKernelGGL(roll_crops_kernel, dim3((IMG * IMG + NT - 1) / NT, (unsigned)n, 2), dim3(NT), 0, (hipStream_t)stream, k);
    APG_TRY(hipGetLastError());
    return APG_OK;
}
