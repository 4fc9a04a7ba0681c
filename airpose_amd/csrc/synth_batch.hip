// Synthetic-data batches (libairpose_grad.so): aerialpeople_crop.__getitem__ (copenet/src/copenet/dsets/aerialpeople.py:81-226) between
// a sample's pickled record and the batch dict, for n samples and both cameras.  The semantics, the draws, the box invariant and the
// three rules that give it are in include/airpose_grad.h.  Restated from the reference:
//   :98-135   the region bb -+ margin clipped to the frame, four uniform offsets in [0, range) drawn in the order ymin side, ymax
//             side, xmin side, xmax side (0 where the range is 0), crop_info = the region, bb = crop centre / principal point - 1
//   :148-177  transform_smpl (utils/utils.py:237-256) of vertices, joints, orientation and translation into each camera,
//             perspective_projection with R = I and t = 0 (utils/geometry.py:63-91): f (x / z, y / z) + c, the joints in crop pixels
//             s * (j2d - (bb + 1) * c), lbs.batch_rodrigues of the 21 body joints
//   :208-211  cam1 = randint(2): per sample, suffix 0 is camera cam1 and suffix 1 the other
//   :125-141, 174 and resize_with_pad (utils/utils.py:214-235): the image, preprocess_px.inc
//
//   synth_sample_kernel   grid = n, APG_SYNTH_THREADS threads: ONE WORKGROUP per sample.  Threads 0 and 1 take camera 0 and 1: the
//     box, its records, the copies of intr and extr, orient_rel and trans_rel, and leave scale and the crop's origin in LDS for the
//     joints; after the barrier thread j, j + 128, .. takes joint j for both cameras and threads < 21 a body joint's rotation.
//   synth_verts_kernel    grid = (ceil(V / 256), n): one thread per vertex, read once, transformed and written for both cameras.
//   synth_crops_kernel    grid = (196, n, 2 suffixes): preprocess_px on the canvas of camera flip ^ s.
// Every kernel recomputes the sample's flip from the same draw, so none waits for another's output except synth_crops_kernel, which
// reads the boxes and flips from memory (it is an entry point of its own).  All fp32 chains are single roundings: this file is
// compiled with -ffp-contract=off (csrc/Makefile); preprocess_px alone contracts, as it does in stem.hip.  No atomic, plain vector
// stores only.  Launch-bound at the reference's sizes: 24 MB move per batch of 64.
#include "grad_internal.h"

#include <cmath>
#include <string>

namespace {

constexpr int NT = APG_SYNTH_THREADS;
constexpr int VT = 256;
constexpr int MAX_N = 65535, MAX_V = 1 << 24, MAX_J = 1 << 16, MAX_SIDE = 1 << 20;
constexpr int IMG = 224;

#include "preprocess_px.inc"

struct SynthArgs {
    int n, V, J, H, W, Hc, Wc, margin, origin, jitter, shuffle;
    float fx, fy;
    uint32_t k0, k1, epoch;
    const int *index, *bb_in;
    const float *intr, *extr, *pose, *verts, *joints, *orient, *trans;
    int *crops, *crop_info, *status, *flip;
    float *bb, *intr_out, *extr_out, *verts_rel, *joints_rel, *orient_rel, *trans_rel, *j2d, *j2d_crop, *pose_rotmat;
};

#include "draws.inc"

__device__ __forceinline__ int sample_flip(const SynthArgs& a, int i) {
    if (!a.shuffle) return 0;
    return (int)(philox((uint32_t)a.index[i], a.epoch, 2u, 0u, a.k0, a.k1).w[0] >> 31);
}

// One axis of the box (include/airpose_grad.h): a0, a1 the record's corners, S the frame's and Sc the canvas's size along it, w0 and
// w1 the two draws.  -> lo, hi the region; p0 < p1 the crop in frame coordinates; 0 <= q0 < q1 <= Sc the crop on the canvas
__device__ __forceinline__ int box_axis(int a0, int a1, int S, int Sc, const SynthArgs& a, uint32_t w0, uint32_t w1, int& lo, int& hi,
                                        int& p0, int& p1, int& q0, int& q1) {
    int st = 0;
    const int c0 = min(max(a0, 0), S), c1 = min(max(a1, 0), S);      // rule 1; from here on everything is in 0 .. 2^21
    if (c0 != a0 || c1 != a1) st |= APG_SYNTH_CLAMPED;
    lo = c0 - a.margin > 0 ? c0 - a.margin : 0;                      // lo <= c0
    hi = c1 + a.margin < S ? c1 + a.margin : S;                      // hi >= c1
    const uint32_t r0 = (uint32_t)(c0 - lo), r1 = (uint32_t)(hi - c1);
    const int o0 = a.jitter && r0 ? (int)__umulhi(w0, r0) : 0;       // in [0, r0)
    const int o1 = a.jitter && r1 ? (int)__umulhi(w1, r1) : 0;
    p0 = lo + o0;
    p1 = hi - o1;
    if (p1 <= p0) {                                                  // rule 2
        p0 = min(p0, S - 1);
        p1 = p0 + 1;
        st |= APG_SYNTH_WIDENED;
    }
    const int base = a.origin == APG_SYNTH_ORIGIN_REGION ? lo : 0;
    q0 = p0 - base;
    q1 = p1 - base;
    if (q0 < 0 || q1 > Sc) {                                         // rule 3
        q0 = min(max(q0, 0), Sc - 1);
        q1 = min(max(q1, q0 + 1), Sc);
        st |= APG_SYNTH_OUTSIDE;
    }
    p0 = q0 + base;
    p1 = q1 + base;
    return st;
}

// rows 0 .. 2 of a 4 x 4 [R | t] applied to a point: ((R0 x + R1 y) + R2 z) + t
__device__ __forceinline__ void rigid(const float* __restrict__ m, float x, float y, float z, float& X, float& Y, float& Z) {
    X = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    Y = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    Z = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
}

__global__ void __launch_bounds__(NT) synth_sample_kernel(const SynthArgs a) {
    __shared__ float s_scale[2], s_ox[2], s_oy[2];
    const int i = blockIdx.x, tid = threadIdx.x, n = a.n;
    const int flip = sample_flip(a, i);
    if (tid < 2) {
        const int c = tid, s = c ^ flip;
        const size_t f = (size_t)s * n + i, g = (size_t)i * 2 + c;   // the output row of suffix s, the input row of camera c
        const int* b = a.bb_in + g * 4;                              // x0, y0, x1, y1
        const U4 d = philox((uint32_t)a.index[i], a.epoch, (uint32_t)c, 0u, a.k0, a.k1);
        int ylo, yhi, xlo, xhi, py0, py1, px0, px1, qy0, qy1, qx0, qx1;
        int st = box_axis(b[1], b[3], a.H, a.Hc, a, d.w[0], d.w[1], ylo, yhi, py0, py1, qy0, qy1);
        st |= box_axis(b[0], b[2], a.W, a.Wc, a, d.w[2], d.w[3], xlo, xhi, px0, px1, qx0, qx1);
        int* cr = a.crops + f * 4;
        cr[0] = qy0; cr[1] = qy1; cr[2] = qx0; cr[3] = qx1;
        int* ci = a.crop_info + f * 4;
        ci[0] = ylo; ci[1] = xlo; ci[2] = yhi; ci[3] = xhi;
        a.status[f] = st;
        const float* K = a.intr + g * 9;
        const float* E = a.extr + g * 16;
        const int bh = qy1 - qy0, bw = qx1 - qx0;
        const float scale = (float)(224.0 / (double)(bh > bw ? bh : bw));                 // preprocess_px's expression
        const float cx = K[2], cy = K[5];
        const float bbx = (float)(px0 + px1) / 2.f / cx - 1.f;       // the sum is exact (< 2^22); one rounding in / and one in -
        const float bby = (float)(py0 + py1) / 2.f / cy - 1.f;
        float* bo = a.bb + f * 3;
        bo[0] = bbx; bo[1] = bby; bo[2] = scale;
        s_scale[c] = scale; s_ox[c] = (bbx + 1.f) * cx; s_oy[c] = (bby + 1.f) * cy;
        float* Ko = a.intr_out + f * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) Ko[k] = K[k];
        float* Eo = a.extr_out + f * 16;
#pragma unroll
        for (int k = 0; k < 16; ++k) Eo[k] = E[k];
        const float* O = a.orient + (size_t)i * 9;
        float* Oo = a.orient_rel + f * 9;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) Oo[r * 3 + k] = (E[r * 4] * O[k] + E[r * 4 + 1] * O[3 + k]) + E[r * 4 + 2] * O[6 + k];
        const float* t = a.trans + (size_t)i * 3;
        float* to = a.trans_rel + f * 3;
        rigid(E, t[0], t[1], t[2], to[0], to[1], to[2]);
        if (c == 0) a.flip[i] = flip;
    }
    __syncthreads();
    for (int j = tid; j < a.J; j += NT) {
        const float* p = a.joints + ((size_t)i * a.J + j) * 3;
        const float x = p[0], y = p[1], z = p[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const size_t g = (size_t)i * 2 + c, o = ((size_t)(c ^ flip) * n + i) * a.J + j;
            const float* K = a.intr + g * 9;
            float X, Y, Z;
            rigid(a.extr + g * 16, x, y, z, X, Y, Z);
            float* q = a.joints_rel + o * 3;
            q[0] = X; q[1] = Y; q[2] = Z;
            const float u = a.fx * (X / Z) + K[2], v = a.fy * (Y / Z) + K[5];
            a.j2d[o * 2] = u; a.j2d[o * 2 + 1] = v;
            a.j2d_crop[o * 2] = s_scale[c] * (u - s_ox[c]);
            a.j2d_crop[o * 2 + 1] = s_scale[c] * (v - s_oy[c]);
        }
    }
    if (tid < 21) {                                                  // lbs.batch_rodrigues of body joint tid
        const float* r = a.pose + (size_t)i * 63 + tid * 3;
        const float rx = r[0], ry = r[1], rz = r[2];
        const float ex = rx + 1e-8f, ey = ry + 1e-8f, ez = rz + 1e-8f;
        const float angle = sqrtf((ex * ex + ey * ey) + ez * ez);
        const float x = rx / angle, y = ry / angle, z = rz / angle;
        const float sn = sinf(angle), c1 = 1.f - cosf(angle);
        // K = [[0, -z, y], [z, 0, -x], [-y, x, 0]]; K K row by column in bmm's order, its products with 0 left out
        const float kk[9] = {-(z * z) - y * y, y * x, z * x, x * y, -(z * z) - x * x, z * y, x * z, y * z, -(y * y) - x * x};
        const float k[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
        float* o = a.pose_rotmat + ((size_t)i * 21 + tid) * 9;
#pragma unroll
        for (int e = 0; e < 9; ++e) o[e] = ((e % 4 == 0 ? 1.f : 0.f) + sn * k[e]) + c1 * kk[e];
    }
}

__global__ void __launch_bounds__(VT) synth_verts_kernel(const SynthArgs a) {
    const int i = blockIdx.y, v = blockIdx.x * VT + threadIdx.x;
    if (v >= a.V) return;
    const int flip = sample_flip(a, i);
    const float* p = a.verts + ((size_t)i * a.V + v) * 3;
    const float x = p[0], y = p[1], z = p[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        float* q = a.verts_rel + (((size_t)(c ^ flip) * a.n + i) * a.V + v) * 3;
        rigid(a.extr + ((size_t)i * 2 + c) * 16, x, y, z, q[0], q[1], q[2]);
    }
}

__global__ void __launch_bounds__(256) synth_crops_kernel(int n, int Hc, int Wc, int bgr, const unsigned char* __restrict__ frames,
                                                          const int* __restrict__ crops, const int* __restrict__ flip,
                                                          float* __restrict__ im, float* __restrict__ scale, int* __restrict__ pad) {
    const int i = blockIdx.y, s = blockIdx.z, px = blockIdx.x * 256 + threadIdx.x;
    const size_t f = (size_t)s * n + i;
    const int* cr = crops + f * 4;
    const int y0 = cr[0], y1 = cr[1], x0 = cr[2], x1 = cr[3];
    if (y0 < 0 || y1 <= y0 || y1 > Hc || x0 < 0 || x1 <= x0 || x1 > Wc) return;           // the whole workgroup
    const int c = (flip[i] & 1) ^ s;
    preprocess_px(frames + ((size_t)c * n + i) * Hc * Wc * 3, Wc, bgr, cr, im + f * 3 * IMG * IMG, scale + f, pad + f * 2, px);
}

}  // namespace

extern "C" int apg_synth_batch(int n, int V, int J, int H, int W, int Hc, int Wc, int margin, int origin, int jitter, int shuffle,
                               float fx, float fy, uint64_t seed, int epoch, const int* index, const int* bb_in, const float* intr,
                               const float* extr, const float* pose, const float* verts, const float* joints, const float* orient,
                               const float* trans, int* crops, int* crop_info, int* status, int* flip, float* bb, float* intr_out,
                               float* extr_out, float* verts_rel, float* joints_rel, float* orient_rel, float* trans_rel, float* j2d,
                               float* j2d_crop, float* pose_rotmat, void* stream) {
    const std::string f = "apg_synth_batch: ";
    const ApgPtr in[] = {{index, "index", 4}, {bb_in, "bb_in", 4}, {intr, "intr", 4}, {extr, "extr", 4}, {pose, "pose", 4},
                         {verts, "verts", 4}, {joints, "joints", 4}, {orient, "orient", 4}, {trans, "trans", 4}};
    const ApgPtr out[] = {{crops, "crops", 4}, {crop_info, "crop_info", 4}, {status, "status", 4}, {flip, "flip", 4}, {bb, "bb", 4},
                          {intr_out, "intr_out", 4}, {extr_out, "extr_out", 4}, {verts_rel, "verts_rel", 4},
                          {joints_rel, "joints_rel", 4}, {orient_rel, "orient_rel", 4}, {trans_rel, "trans_rel", 4}, {j2d, "j2d", 4},
                          {j2d_crop, "j2d_crop", 4}, {pose_rotmat, "pose_rotmat", 4}};
    if (int rc = apg_check_ptrs(f, in, 9)) return rc;
    if (int rc = apg_check_ptrs(f, out, 14)) return rc;
    if (n < 1 || n > MAX_N) return apg_fail(APG_EINVAL, f + "n must be in 1 .. " + std::to_string(MAX_N));
    if (V < 1 || V > MAX_V) return apg_fail(APG_EINVAL, f + "V must be in 1 .. " + std::to_string(MAX_V));
    if (J < 1 || J > MAX_J) return apg_fail(APG_EINVAL, f + "J must be in 1 .. " + std::to_string(MAX_J));
    const struct { int v; const char* name; } sides[] = {{H, "H"}, {W, "W"}, {Hc, "Hc"}, {Wc, "Wc"}};
    for (const auto& s : sides)
        if (s.v < 1 || s.v > MAX_SIDE) return apg_fail(APG_EINVAL, f + s.name + " must be in 1 .. " + std::to_string(MAX_SIDE));
    if (margin < 0 || margin > MAX_SIDE) return apg_fail(APG_EINVAL, f + "margin must be in 0 .. " + std::to_string(MAX_SIDE));
    if (origin != APG_SYNTH_ORIGIN_REGION && origin != APG_SYNTH_ORIGIN_FRAME)
        return apg_fail(APG_EINVAL, f + "origin must be APG_SYNTH_ORIGIN_REGION (0) or APG_SYNTH_ORIGIN_FRAME (1)");
    if (jitter != 0 && jitter != 1) return apg_fail(APG_EINVAL, f + "jitter must be 0 or 1");
    if (shuffle != 0 && shuffle != 1) return apg_fail(APG_EINVAL, f + "shuffle must be 0 or 1");
    if (!std::isfinite(fx) || !std::isfinite(fy)) return apg_fail(APG_EINVAL, f + "fx and fy must be finite");
    for (const auto& o : out)
        for (const auto& i : in)
            if (o.p == i.p) return apg_fail(APG_EINVAL, f + o.name + " must not be " + i.name);
    const SynthArgs k = {n, V, J, H, W, Hc, Wc, margin, origin, jitter, shuffle, fx, fy, (uint32_t)seed, (uint32_t)(seed >> 32),
                         (uint32_t)epoch, index, bb_in, intr, extr, pose, verts, joints, orient, trans, crops, crop_info, status, flip,
                         bb, intr_out, extr_out, verts_rel, joints_rel, orient_rel, trans_rel, j2d, j2d_crop, pose_rotmat};
    hipLaunchKernelGGL(synth_sample_kernel, dim3((unsigned)n), dim3(NT), 0, (hipStream_t)stream, k);
    APG_TRY(hipGetLastError());
    hipLaunchKernelGGL(synth_verts_kernel, dim3((unsigned)((V + VT - 1) / VT), (unsigned)n), dim3(VT), 0, (hipStream_t)stream, k);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

extern "C" int apg_synth_crops(int n, int Hc, int Wc, int bgr, const unsigned char* frames, const int* crops, const int* flip,
                               float* im, float* scale, int* pad, void* stream) {
    const std::string f = "apg_synth_crops: ";
    if (!frames) return apg_fail(APG_EINVAL, f + "frames is NULL");
    const ApgPtr ps[] = {{crops, "crops", 4}, {flip, "flip", 4}, {im, "im", 4}, {scale, "scale", 4}, {pad, "pad", 4}};
    if (int rc = apg_check_ptrs(f, ps, 5)) return rc;
    if (n < 1 || n > MAX_N) return apg_fail(APG_EINVAL, f + "n must be in 1 .. " + std::to_string(MAX_N));
    if (Hc < 1 || Hc > MAX_SIDE) return apg_fail(APG_EINVAL, f + "Hc must be in 1 .. " + std::to_string(MAX_SIDE));
    if (Wc < 1 || Wc > MAX_SIDE) return apg_fail(APG_EINVAL, f + "Wc must be in 1 .. " + std::to_string(MAX_SIDE));
    if (bgr != 0 && bgr != 1) return apg_fail(APG_EINVAL, f + "bgr must be 0 or 1");
    if ((const void*)im == (const void*)frames) return apg_fail(APG_EINVAL, f + "im must not be frames");
    hipLaunchKernelGGL(synth_crops_kernel, dim3((IMG * IMG + 255) / 256, (unsigned)n, 2), dim3(256), 0, (hipStream_t)stream, n, Hc, Wc,
                       bgr, frames, crops, flip, im, scale, pad);
    APG_TRY(hipGetLastError());
    return APG_OK;
}
