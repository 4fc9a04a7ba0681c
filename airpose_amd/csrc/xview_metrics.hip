// Cross-view metrics for gfx950 (libairpose_grad.so): how well the two views of a calibrated pair agree on one body, without any
// ground truth -- the gaps between the views' joints, vertices, translations and rotations once each is carried into the world
// frame, the confidence-weighted reprojection error against the detections, and the distance of each view's joints from the point
// the two detections triangulate to.  The semantics are in include/airpose_grad.h.
//
//   xview_main_kernel     grid = B * nchunk, NT = 256 threads; nchunk = max(1, ceil(V / 1024)): one workgroup per (sample, chunk of
//     1024 vertices).  Every thread holds the sample's two 3 x 4 transforms in registers as doubles (24 uniform loads) and takes the
//     skip decision itself, so no barrier stands in front of the vertex loads.
//     vertices: thread t takes the points t, t + NT, t + 2 NT, t + 3 NT of its chunk.  A point is 12 bytes and a sample's base only
//       4-byte aligned (V = 10475: a stride of 31425 floats), so a lane loads its point as three dwords and a wave covers 768
//       contiguous bytes per view, as in eval_align.hip.  Per point, in fp64: w_v = R_v^T (p_v - o_v) with o = t (world) or the root,
//       the difference of the two rounded to float once per component, norm3 in fp32, added in fp64 in point order; wg_sum
//       (metric_common.inc) over the workgroup; the chunk's two sums go to the workspace.
//     chunk 0 also takes everything that is small: the joints (thread i, i + NT, ..), the translation (thread 0), the 22 rotations,
//       the 22 reprojections per view and the 22 triangulations (thread j < 22), one wg_sum of all of them, and thread 0 writes the
//       sample's 24 values to the workspace.  A skipped sample writes skipped = 1 and zeros.
//   xview_reduce_kernel   one workgroup of NT threads: thread t takes the samples t, t + NT, .. in order (a sample's chunks in chunk
//     order, divided by V), writes the per-sample outputs, adds its samples in fp64; wg_sum; ONE add per slot into the accumulator.
//   xview_tri_kernel      apg_xview_triangulate: a thread per (sample, joint) on the same device function.
//
// Determinism.  No atomics and no arrival counter; the partition is a function of (B, V) alone.  Plain vector stores only.
#include "grad_internal.h"

#include <string>

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int PPT = 4;                   // points per thread
constexpr int CH = NT * PPT;             // points per chunk
constexpr int NJ = 22;                   // the body joints: rotations, reprojection, triangulation
constexpr int ACC = APG_XVIEW_ACC;
constexpr int NS = ACC - 2;              // sums per sample: accumulator slots 1 .. 24
constexpr int PS = APG_XVIEW_PER_SAMPLE;
constexpr int PER = APG_XVIEW_PER_VIEW;
constexpr double ORTHO_GATE = 1e-3;      // max |R^T R - I| above which a sample is skipped (a design constant: the header)
constexpr double DEG = 57.29577951308232087679815481410517;

// index q of a sum = accumulator slot q + 1
enum { Q_SKIP = 0, Q_JW, Q_JR, Q_NROOT, Q_VW, Q_VR, Q_NVERT, Q_NVROOT, Q_TRANS, Q_NTRANS, Q_ORIENT, Q_POSE, Q_NROT, Q_RP0, Q_RP1,
       Q_RS0, Q_RS1, Q_RN0, Q_RN1, Q_NRP, Q_TRI0, Q_TRI1, Q_TRIN, Q_NTRI };
static_assert(Q_NTRI + 1 == NS, "the sums and the accumulator's layout");

// per-view table entries
enum { T_J = 0, T_E, T_V, T_ROOT, T_TRANS, T_ROT, T_J2D, T_KP, T_K };
static_assert(T_K + 1 == PER, "the per-view table");

struct XArgs {
    int B, nj, V, nchunk;
    int rot_aa, has_root, has_trans, has_rot, has_reproj, has_tri;
    long long stride[PER];                               // floats from one sample to the next, per table entry
    const float* in[2][PER];
    double min_sin2;
    float* per_sample;                                   // (B, PS) or NULL
    float* tri;                                          // (B, NJ, 4) or NULL
    double* part_s;                                      // [sample][NS]
    double* part_v;                                      // [sample][chunk][2]
    double* acc;
};

#include "metric_common.inc"
#include "rot_aa.inc"                    // aa_to_rotmat

struct Cam { double R[9], t[3]; };       // world -> camera: x_cam = R x_world + t

__device__ __forceinline__ bool fin(double x) { return fabs(x) <= 1.79769313486231570815e308; }      // false for NaN and inf

// rows 0 .. 2 of a (3 or 4) x 4 row-major matrix; -> whether the sample may be scored with it
__device__ __forceinline__ bool load_cam(const float* e, Cam& c) {
    bool ok = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c.R[r * 3 + k] = (double)e[r * 4 + k], ok = ok && fin(c.R[r * 3 + k]);
        c.t[r] = (double)e[r * 4 + 3], ok = ok && fin(c.t[r]);
    }
    double dev = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            const double g = ((c.R[i] * c.R[j] + c.R[3 + i] * c.R[3 + j]) + c.R[6 + i] * c.R[6 + j]) - (i == j ? 1.0 : 0.0);
            dev = fabs(g) > dev ? fabs(g) : dev;
        }
    return ok && dev <= ORTHO_GATE;
}

// w = R^T (p - o)
__device__ __forceinline__ void carry(const Cam& c, double p0, double p1, double p2, const double* o, double* w) {
    const double d0 = p0 - o[0], d1 = p1 - o[1], d2 = p2 - o[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) w[r] = (c.R[r] * d0 + c.R[3 + r] * d1) + c.R[6 + r] * d2;
}

// |R_0^T (p - o0) - R_1^T (q - o1)|
__device__ __forceinline__ double gap(const Cam& c0, const Cam& c1, const float* p, const float* q, const double* o0, const double* o1) {
    double w0[3], w1[3];
    carry(c0, (double)p[0], (double)p[1], (double)p[2], o0, w0);
    carry(c1, (double)q[0], (double)q[1], (double)q[2], o1, w1);
    return (double)norm3((float)(w0[0] - w1[0]), (float)(w0[1] - w1[1]), (float)(w0[2] - w1[2]));
}

// the geodesic angle of D = A^T B in degrees: atan2(|axial vector of D|, tr D - 1)
__device__ __forceinline__ double angle_deg(const double* A, const double* B) {
    double D[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) D[i * 3 + j] = (A[i] * B[j] + A[3 + i] * B[3 + j]) + A[6 + i] * B[6 + j];
    const double x = D[7] - D[5], y = D[2] - D[6], z = D[3] - D[1];
    return atan2(sqrt((x * x + y * y) + z * z), ((D[0] + D[4]) + D[8]) - 1.0) * DEG;
}

// lstsq_triangulation for two cameras: kp = x, y, confidence; K = the 3 x 3 intrinsics, of which fx, cx, fy, cy are read
__device__ __forceinline__ bool triangulate(const Cam& c0, const Cam& c1, const float* kp0, const float* kp1, const float* K0,
                                            const float* K1, double min_sin2, double* T) {
    double M[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, y[3] = {0.0, 0.0, 0.0}, ray[2][3];     // M: 00 01 02 11 12 22
    bool ok = true;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const Cam& c = v ? c1 : c0;
        const float* kp = v ? kp1 : kp0;
        const float* K = v ? K1 : K0;
        const double px = (double)kp[0], py = (double)kp[1], conf = (double)kp[2];
        ok = ok && fin(px) && fin(py) && fin(conf) && conf > 0.0;
        const double n[2] = {(px - (double)K[2]) / (double)K[0], (py - (double)K[5]) / (double)K[4]};
        ok = ok && fin(n[0]) && fin(n[1]);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const double a0 = n[r] * c.R[6] - c.R[r * 3], a1 = n[r] * c.R[7] - c.R[r * 3 + 1], a2 = n[r] * c.R[8] - c.R[r * 3 + 2];
            const double b = c.t[r] - c.t[2] * n[r];
            M[0] += a0 * a0, M[1] += a0 * a1, M[2] += a0 * a2, M[3] += a1 * a1, M[4] += a1 * a2, M[5] += a2 * a2;
            y[0] += a0 * b, y[1] += a1 * b, y[2] += a2 * b;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) ray[v][r] = (c.R[r] * n[0] + c.R[3 + r] * n[1]) + c.R[6 + r];
    }
    const double c00 = M[3] * M[5] - M[4] * M[4], c01 = M[2] * M[4] - M[1] * M[5], c02 = M[1] * M[4] - M[2] * M[3];
    const double c11 = M[0] * M[5] - M[2] * M[2], c12 = M[1] * M[2] - M[0] * M[4], c22 = M[0] * M[3] - M[1] * M[1];
    const double det = (M[0] * c00 + M[1] * c01) + M[2] * c02;
    T[0] = ((c00 * y[0] + c01 * y[1]) + c02 * y[2]) / det;
    T[1] = ((c01 * y[0] + c11 * y[1]) + c12 * y[2]) / det;
    T[2] = ((c02 * y[0] + c12 * y[1]) + c22 * y[2]) / det;
    const double* d0 = ray[0];
    const double* d1 = ray[1];
    const double cx = d0[1] * d1[2] - d0[2] * d1[1], cy = d0[2] * d1[0] - d0[0] * d1[2], cz = d0[0] * d1[1] - d0[1] * d1[0];
    const double s2 = ((cx * cx + cy * cy) + cz * cz) /
                      (((d0[0] * d0[0] + d0[1] * d0[1]) + d0[2] * d0[2]) * ((d1[0] * d1[0] + d1[1] * d1[1]) + d1[2] * d1[2]));
    return ok && s2 >= min_sin2 && fin(T[0]) && fin(T[1]) && fin(T[2]);
}

__global__ void __launch_bounds__(NT) xview_main_kernel(const XArgs a) {
    __shared__ double red[(NT / 64) * NS];
    __shared__ double tot[NS];
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)a.nchunk);                // blockIdx.x = b * nchunk + chunk < B * nchunk
    const int chunk = (int)(blockIdx.x - (unsigned)b * (unsigned)a.nchunk);
    const size_t sb = (size_t)b;
    Cam c0, c1;
    const bool ok0 = load_cam(a.in[0][T_E] + sb * (size_t)a.stride[T_E], c0);
    const bool ok1 = load_cam(a.in[1][T_E] + sb * (size_t)a.stride[T_E], c1);
    const bool ok = ok0 && ok1;                                          // (uniform over the workgroup)
    double r0[3] = {0.0, 0.0, 0.0}, r1[3] = {0.0, 0.0, 0.0};
    if (a.has_root) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r0[k] = (double)a.in[0][T_ROOT][sb * (size_t)a.stride[T_ROOT] + k];
            r1[k] = (double)a.in[1][T_ROOT][sb * (size_t)a.stride[T_ROOT] + k];
        }
    }

    if (a.V > 0) {
        double e[2] = {0.0, 0.0};
        if (ok) {
            const float* P = a.in[0][T_V] + sb * (size_t)a.stride[T_V];
            const float* Q = a.in[1][T_V] + sb * (size_t)a.stride[T_V];
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const int i = chunk * CH + k * NT + tid;                 // a wave's 64 points are 768 contiguous bytes per view
                if (i < a.V) {
                    e[0] += gap(c0, c1, P + (size_t)i * 3, Q + (size_t)i * 3, c0.t, c1.t);
                    if (a.has_root) e[1] += gap(c0, c1, P + (size_t)i * 3, Q + (size_t)i * 3, r0, r1);
                }
            }
        }
        wg_sum<NT, 2>(e, red, tot);
        if (tid < 2) a.part_v[(size_t)blockIdx.x * 2 + tid] = tot[tid];
    }
    if (chunk != 0) return;                                              // (uniform)

    double s[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = 0.0;
    float* tri = a.tri ? a.tri + (sb * NJ + (size_t)tid) * 4 : nullptr;  // thread tid < NJ owns row tid
    if (ok) {
        const float* J0 = a.in[0][T_J] + sb * (size_t)a.stride[T_J];
        const float* J1 = a.in[1][T_J] + sb * (size_t)a.stride[T_J];
        for (int i = tid; i < a.nj; i += NT) {
            s[Q_JW] += gap(c0, c1, J0 + (size_t)i * 3, J1 + (size_t)i * 3, c0.t, c1.t);
            if (a.has_root) s[Q_JR] += gap(c0, c1, J0 + (size_t)i * 3, J1 + (size_t)i * 3, r0, r1);
        }
        if (a.has_trans && tid == 0)
            s[Q_TRANS] = gap(c0, c1, a.in[0][T_TRANS] + sb * (size_t)a.stride[T_TRANS], a.in[1][T_TRANS] + sb * (size_t)a.stride[T_TRANS],
                             c0.t, c1.t);
        if (tid < NJ) {
            if (a.has_rot) {
                double Q[2][9];
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    const float* src = a.in[v][T_ROT] + sb * (size_t)a.stride[T_ROT] + (size_t)tid * (a.rot_aa ? 3 : 9);
                    float m[9];
                    if (a.rot_aa) {
                        aa_to_rotmat(src[0], src[1], src[2], m);
                    } else {
#pragma unroll
                        for (int k = 0; k < 9; ++k) m[k] = src[k];
                    }
#pragma unroll
                    for (int k = 0; k < 9; ++k) Q[v][k] = (double)m[k];
                }
                if (tid == 0) {                                          // the root's rotation, carried into the world: R_v^T Q_v
                    double A[2][9];
#pragma unroll
                    for (int v = 0; v < 2; ++v) {
                        const Cam& c = v ? c1 : c0;
#pragma unroll
                        for (int i = 0; i < 3; ++i)
#pragma unroll
                            for (int j = 0; j < 3; ++j)
                                A[v][i * 3 + j] = (c.R[i] * Q[v][j] + c.R[3 + i] * Q[v][3 + j]) + c.R[6 + i] * Q[v][6 + j];
                    }
                    s[Q_ORIENT] = angle_deg(A[0], A[1]);
                } else {
                    s[Q_POSE] = angle_deg(Q[0], Q[1]);
                }
            }
            if (a.has_reproj) {
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    const float* kp = a.in[v][T_KP] + sb * (size_t)a.stride[T_KP] + (size_t)tid * 3;
                    const float* pr = a.in[v][T_J2D] + sb * (size_t)a.stride[T_J2D] + (size_t)tid * 2;
                    const double x = (double)kp[0], y = (double)kp[1], conf = (double)kp[2];
                    if (fin(x) && fin(y) && fin(conf) && conf > 0.0) {
                        const float dx = (float)((double)pr[0] - x), dy = (float)((double)pr[1] - y);
                        s[Q_RP0 + v] = conf * (double)sqrtf(fmaf(dy, dy, dx * dx));
                        s[Q_RS0 + v] = conf;
                        s[Q_RN0 + v] = 1.0;
                    }
                }
            }
            if (a.has_tri) {
                double T[3];
                const bool valid = triangulate(c0, c1, a.in[0][T_KP] + sb * (size_t)a.stride[T_KP] + (size_t)tid * 3,
                                               a.in[1][T_KP] + sb * (size_t)a.stride[T_KP] + (size_t)tid * 3,
                                               a.in[0][T_K] + sb * (size_t)a.stride[T_K], a.in[1][T_K] + sb * (size_t)a.stride[T_K],
                                               a.min_sin2, T);
                if (valid) {
                    double w[3];
                    carry(c0, (double)J0[tid * 3], (double)J0[tid * 3 + 1], (double)J0[tid * 3 + 2], c0.t, w);
                    s[Q_TRI0] = (double)norm3((float)(w[0] - T[0]), (float)(w[1] - T[1]), (float)(w[2] - T[2]));
                    carry(c1, (double)J1[tid * 3], (double)J1[tid * 3 + 1], (double)J1[tid * 3 + 2], c1.t, w);
                    s[Q_TRI1] = (double)norm3((float)(w[0] - T[0]), (float)(w[1] - T[1]), (float)(w[2] - T[2]));
                    s[Q_TRIN] = 1.0;
                }
                if (tri) tri[0] = valid ? (float)T[0] : 0.f, tri[1] = valid ? (float)T[1] : 0.f, tri[2] = valid ? (float)T[2] : 0.f, tri[3] = valid ? 1.f : 0.f;
            }
        }
    } else if (tid < NJ && tri) {
        tri[0] = 0.f, tri[1] = 0.f, tri[2] = 0.f, tri[3] = 0.f;
    }
    wg_sum<NT, NS>(s, red, tot);
    if (tid == 0) {
        double* out = a.part_s + sb * NS;
#pragma unroll
        for (int k = 0; k < NS; ++k) out[k] = 0.0;
        if (!ok) {
            out[Q_SKIP] = 1.0;
            return;
        }
        out[Q_JW] = tot[Q_JW] / (double)a.nj;
        out[Q_JR] = a.has_root ? tot[Q_JR] / (double)a.nj : 0.0;
        out[Q_NROOT] = a.has_root ? 1.0 : 0.0;
        out[Q_NVERT] = a.V > 0 ? 1.0 : 0.0;
        out[Q_NVROOT] = a.V > 0 && a.has_root ? 1.0 : 0.0;
        out[Q_TRANS] = tot[Q_TRANS], out[Q_NTRANS] = a.has_trans ? 1.0 : 0.0;
        out[Q_ORIENT] = tot[Q_ORIENT], out[Q_POSE] = tot[Q_POSE] / (double)(NJ - 1), out[Q_NROT] = a.has_rot ? 1.0 : 0.0;
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const double sc = tot[Q_RS0 + v];
            out[Q_RP0 + v] = sc > 0.0 ? tot[Q_RP0 + v] / sc : 0.0;
            out[Q_RS0 + v] = sc > 0.0 ? 1.0 : 0.0;
            out[Q_RN0 + v] = tot[Q_RN0 + v];
        }
        out[Q_NRP] = a.has_reproj ? 1.0 : 0.0;
        out[Q_TRI0] = tot[Q_TRI0], out[Q_TRI1] = tot[Q_TRI1], out[Q_TRIN] = tot[Q_TRIN], out[Q_NTRI] = a.has_tri ? 1.0 : 0.0;
    }
}

__global__ void __launch_bounds__(NT) xview_reduce_kernel(const XArgs a) {
    __shared__ double red[(NT / 64) * NS];
    __shared__ double tot[NS];
    const int tid = threadIdx.x;
    double v[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = 0.0;
    for (int b = tid; b < a.B; b += NT) {
        double x[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) x[k] = a.part_s[(size_t)b * NS + k];
        if (a.V > 0) {
            double vw = 0.0, vr = 0.0;
            for (int c = 0; c < a.nchunk; ++c) {
                vw += a.part_v[((size_t)b * (size_t)a.nchunk + (size_t)c) * 2];
                vr += a.part_v[((size_t)b * (size_t)a.nchunk + (size_t)c) * 2 + 1];
            }
            x[Q_VW] = vw / (double)a.V, x[Q_VR] = vr / (double)a.V;
        }
        if (a.per_sample) {
            float* o = a.per_sample + (size_t)b * PS;
            o[0] = (float)x[Q_SKIP], o[1] = (float)x[Q_JW], o[2] = (float)x[Q_JR], o[3] = (float)x[Q_VW], o[4] = (float)x[Q_VR];
            o[5] = (float)x[Q_TRANS], o[6] = (float)x[Q_ORIENT], o[7] = (float)x[Q_POSE];
            o[8] = (float)x[Q_RP0], o[9] = (float)x[Q_RP1], o[10] = (float)x[Q_RN0], o[11] = (float)x[Q_RN1];
            o[12] = x[Q_TRIN] > 0.0 ? (float)(x[Q_TRI0] / x[Q_TRIN]) : 0.f;
            o[13] = x[Q_TRIN] > 0.0 ? (float)(x[Q_TRI1] / x[Q_TRIN]) : 0.f;
            o[14] = (float)x[Q_TRIN], o[15] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) v[k] += x[k];
    }
    wg_sum<NT, NS>(v, red, tot);
    if (tid < NS) a.acc[1 + tid] += tot[tid];
    else if (tid == NS) a.acc[0] += (double)a.B;
}

struct TriArgs {
    int B, J;
    const float *kp[2], *K[2], *e[2];
    double min_sin2;
    float* out;
};

__global__ void __launch_bounds__(NT) xview_tri_kernel(const TriArgs a) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= (size_t)a.B * (size_t)a.J) return;
    const size_t b = i / (size_t)a.J;
    Cam c0, c1;
    const bool ok0 = load_cam(a.e[0] + b * 16, c0);
    const bool ok1 = load_cam(a.e[1] + b * 16, c1);
    double T[3];
    const bool valid = triangulate(c0, c1, a.kp[0] + i * 3, a.kp[1] + i * 3, a.K[0] + b * 9, a.K[1] + b * 9, a.min_sin2, T) && ok0 && ok1;
    float* o = a.out + i * 4;
    o[0] = valid ? (float)T[0] : 0.f, o[1] = valid ? (float)T[1] : 0.f, o[2] = valid ? (float)T[2] : 0.f, o[3] = valid ? 1.f : 0.f;
}

constexpr int MAX_B = 1 << 22, MAX_N = 1 << 24, MAX_J = 1 << 16;

inline int64_t nchunks(int N) { return N > 0 ? ((int64_t)N + CH - 1) / CH : 1; }
inline bool sin2_ok(double x) { return x >= 0.0 && x <= 1.0; }           // false for NaN

}  // namespace

extern "C" {

int64_t apg_xview_acc_doubles(void) { return ACC; }

int64_t apg_xview_workspace_bytes(int B, int views, int N) {
    if (B < 1 || B > MAX_B || N < 0 || N > MAX_N || views != 2) return -1;
    if ((int64_t)B * nchunks(N) > 0x7fffffffll) return -1;
    return (int64_t)B * (NS + 2 * nchunks(N)) * (int64_t)sizeof(double);
}

int apg_xview_update(int B, int views, int n_joints, int N, int flags, const int64_t* strides, const void* const* per_view,
                     double min_sin2, float* per_sample, float* tri, double* acc, void* workspace, int64_t workspace_bytes,
                     void* stream) {
    const std::string f = "apg_xview_update: ";
    static const char* const name[PER] = {"joints", "extr", "vertices", "root", "trans", "rot", "j2d", "keypoints", "intr"};
    const MetricChecks m = {f, 2, per_view, PER, 2, name, acc, workspace, workspace_bytes, apg_xview_workspace_bytes(B, 2, N),
                            "apg_xview_workspace_bytes"};
    if (B < 1 || B > MAX_B) return apg_fail(APG_EINVAL, f + "B must be in 1 .. " + std::to_string(MAX_B));
    if (views != 2) return apg_fail(APG_EINVAL, f + "views must be 2: the metric compares two views");
    if (n_joints < 1 || n_joints > MAX_J) return apg_fail(APG_EINVAL, f + "n_joints must be in 1 .. " + std::to_string(MAX_J));
    if (N < 0 || N > MAX_N) return apg_fail(APG_EINVAL, f + "N must be in 0 .. " + std::to_string(MAX_N));
    if (m.need < 0) return apg_fail(APG_EINVAL, f + "B * ceil(N / " + std::to_string(CH) + ") must be below 2^31");
    if (flags != APG_XVIEW_ANGLE_AXIS && flags != APG_XVIEW_ROTMAT) return apg_fail(APG_EINVAL, f + "flags must be APG_XVIEW_ANGLE_AXIS or APG_XVIEW_ROTMAT");
    if (!(sin2_ok(min_sin2))) return apg_fail(APG_EINVAL, f + "min_sin2 must be in 0 .. 1");
    if (!strides) return apg_fail(APG_EINVAL, f + "the strides table is NULL");
    if (int rc = m.table_ok()) return rc;
    if (int rc = m.sinks_ok()) return rc;
    for (int v = 0; v < 2; ++v)
        if (int rc = m.view_ok(v)) return rc;
    for (int k = 2; k < PER; ++k) {
        const bool h0 = per_view[k] != nullptr, h1 = per_view[PER + k] != nullptr;
        if (h0 != h1) return apg_fail(APG_EINVAL, f + name[k] + " of view " + std::to_string(h0 ? 0 : 1) + " is given for one view only");
    }
    const bool has_v = per_view[T_V], has_root = per_view[T_ROOT], has_trans = per_view[T_TRANS], has_rot = per_view[T_ROT];
    const bool has_j2d = per_view[T_J2D], has_kp = per_view[T_KP], has_k = per_view[T_K];
    if (has_v && N == 0) return apg_fail(APG_EINVAL, f + "vertices are given with N = 0");
    if (!has_v && N > 0) return apg_fail(APG_EINVAL, f + "N = " + std::to_string(N) + " without vertices");
    if (has_j2d && !has_kp) return apg_fail(APG_EINVAL, f + "j2d is given without keypoints");
    if (has_kp && !has_j2d && !has_k) return apg_fail(APG_EINVAL, f + "keypoints are given without j2d or intr");
    if (has_k && !has_kp) return apg_fail(APG_EINVAL, f + "intr is given without keypoints");
    if (tri && !has_k) return apg_fail(APG_EINVAL, f + "tri is asked for without intr and keypoints");
    const int64_t need_j = 3 * (int64_t)(has_k && n_joints < NJ ? NJ : n_joints);
    const int64_t least[PER] = {need_j, 12, 3 * (int64_t)N, 3, 3, NJ * (flags == APG_XVIEW_ROTMAT ? 9 : 3), NJ * 2, NJ * 3, 9};
    const bool given[PER] = {true, true, has_v, has_root, has_trans, has_rot, has_j2d, has_kp, has_k};
    for (int k = 0; k < PER; ++k)
        if (given[k] && strides[k] < least[k])
            return apg_fail(APG_EINVAL, f + name[k] + "_stride must be at least " + std::to_string(least[k]) + " floats");
    if ((uintptr_t)per_sample & 3) return apg_fail(APG_EINVAL, f + "per_sample is not 4-byte aligned");
    if ((uintptr_t)tri & 3) return apg_fail(APG_EINVAL, f + "tri is not 4-byte aligned");
    if (int rc = m.sizes_ok()) return rc;

    XArgs a = {};
    a.B = B, a.nj = n_joints, a.V = N, a.nchunk = (int)nchunks(N);
    a.rot_aa = flags == APG_XVIEW_ANGLE_AXIS, a.has_root = has_root, a.has_trans = has_trans, a.has_rot = has_rot;
    a.has_reproj = has_j2d, a.has_tri = has_k;
    for (int k = 0; k < PER; ++k) {
        a.stride[k] = given[k] ? strides[k] : 0;
        a.in[0][k] = (const float*)per_view[k], a.in[1][k] = (const float*)per_view[PER + k];
    }
    a.min_sin2 = min_sin2, a.per_sample = per_sample, a.tri = tri;
    a.part_s = (double*)workspace, a.part_v = a.part_s + (size_t)B * NS, a.acc = acc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(xview_main_kernel, dim3((unsigned)B * (unsigned)a.nchunk), dim3(NT), 0, st, a);
    APG_TRY(hipGetLastError());
    hipLaunchKernelGGL(xview_reduce_kernel, dim3(1), dim3(NT), 0, st, a);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

int apg_xview_triangulate(int B, int J, const float* kp0, const float* kp1, const float* intr0, const float* intr1, const float* extr0,
                          const float* extr1, double min_sin2, float* out, void* stream) {
    const std::string f = "apg_xview_triangulate: ";
    if (B < 1 || B > MAX_B) return apg_fail(APG_EINVAL, f + "B must be in 1 .. " + std::to_string(MAX_B));
    if (J < 1 || J > MAX_J) return apg_fail(APG_EINVAL, f + "J must be in 1 .. " + std::to_string(MAX_J));
    if (!(sin2_ok(min_sin2))) return apg_fail(APG_EINVAL, f + "min_sin2 must be in 0 .. 1");
    const void* const p[7] = {kp0, kp1, intr0, intr1, extr0, extr1, out};
    static const char* const name[7] = {"kp0", "kp1", "intr0", "intr1", "extr0", "extr1", "out"};
    for (int k = 0; k < 7; ++k) {
        if (!p[k]) return apg_fail(APG_EINVAL, f + name[k] + " is NULL");
        if ((uintptr_t)p[k] & 3) return apg_fail(APG_EINVAL, f + name[k] + " is not 4-byte aligned");
    }
    TriArgs a = {B, J, {kp0, kp1}, {intr0, intr1}, {extr0, extr1}, min_sin2, out};
    const int64_t n = (int64_t)B * J;
    hipLaunchKernelGGL(xview_tri_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, a);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

}  // extern "C"
