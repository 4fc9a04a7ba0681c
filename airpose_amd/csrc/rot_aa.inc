// The 3-vector and the rotation matrix -> axis-angle map with its adjoint, once, for fitting.hip (libairpose_hip.so: the fitter's
// decoder output) and loss_real_grad.hip (libairpose_grad.so: the VPoser prior's way in and back), and the axis-angle -> rotation
// matrix map of eval_metrics.hip and xview_metrics.hip.  Included inside each file's unnamed namespace.

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

// rotation matrix (row-major r[9]) -> axis-angle, tgm 0.1.2 (see smplx.hip rotmat_to_angle_axis_kernel), keeping what
// the adjoint needs
struct AA { V3 aa; float q[4], t, s, w, x, y, z; int br; };
__device__ __forceinline__ AA aa_fwd(const float* r) {
    AA a;
    const float t00 = r[0], t10 = r[1], t20 = r[2], t01 = r[3], t11 = r[4], t21 = r[5], t02 = r[6], t12 = r[7], t22 = r[8];
    if (t22 < 1e-6f) {
        if (t00 > t11) { a.br = 0; a.t = 1 + t00 - t11 - t22; a.q[0] = t12 - t21; a.q[1] = a.t; a.q[2] = t01 + t10; a.q[3] = t20 + t02; }
        else           { a.br = 1; a.t = 1 - t00 + t11 - t22; a.q[0] = t20 - t02; a.q[1] = t01 + t10; a.q[2] = a.t; a.q[3] = t12 + t21; }
    } else {
        if (t00 < -t11) { a.br = 2; a.t = 1 - t00 - t11 + t22; a.q[0] = t01 - t10; a.q[1] = t20 + t02; a.q[2] = t12 + t21; a.q[3] = a.t; }
        else            { a.br = 3; a.t = 1 + t00 + t11 + t22; a.q[0] = a.t; a.q[1] = t12 - t21; a.q[2] = t20 - t02; a.q[3] = t01 - t10; }
    }
    a.s = 0.5f / sqrtf(a.t);
    a.w = a.q[0] * a.s; a.x = a.q[1] * a.s; a.y = a.q[2] * a.s; a.z = a.q[3] * a.s;
    const float ss = a.x * a.x + a.y * a.y + a.z * a.z, sn = sqrtf(ss);
    const float two_theta = 2.0f * (a.w < 0.f ? atan2f(-sn, -a.w) : atan2f(sn, a.w));
    const float k = ss > 0.f ? two_theta / sn : 2.0f;
    a.aa = v3(a.x * k, a.y * k, a.z * k);
    return a;
}
// d(loss)/d(aa) -> d(loss)/d(R) (row-major dr[9], overwritten)
__device__ __forceinline__ void aa_bwd(const AA& a, V3 daa, float* dr) {
    const float ss = a.x * a.x + a.y * a.y + a.z * a.z, sn = sqrtf(ss);
    float dw = 0.f;
    V3 dxyz;
    if (ss > 0.f) {
        const float T = 2.0f * (a.w < 0.f ? atan2f(-sn, -a.w) : atan2f(sn, a.w)), k = T / sn;
        const float dk = daa.x * a.x + daa.y * a.y + daa.z * a.z;
        dxyz = k * daa;
        const float dT = dk / sn;
        float dsn = -dk * T / ss;
        const float den = ss + a.w * a.w;
        dsn += 2.f * dT * a.w / den;
        dw = -2.f * dT * sn / den;
        const float dss = dsn / (2.f * sn);
        dxyz = dxyz + (2.f * dss) * v3(a.x, a.y, a.z);
    } else {
        dxyz = 2.f * daa;
    }
    const float dq[4] = {dw * a.s, dxyz.x * a.s, dxyz.y * a.s, dxyz.z * a.s};
    const float ds = dw * a.q[0] + dxyz.x * a.q[1] + dxyz.y * a.q[2] + dxyz.z * a.q[3];
    float dt = -ds * a.s / (2.f * a.t);
    float d00 = 0, d10 = 0, d20 = 0, d01 = 0, d11 = 0, d21 = 0, d02 = 0, d12 = 0, d22 = 0;   // d/d t_ab (t_ab = r[b][a])
    switch (a.br) {
        case 0: dt += dq[1]; d12 += dq[0]; d21 -= dq[0]; d01 += dq[2]; d10 += dq[2]; d20 += dq[3]; d02 += dq[3];
                d00 += dt; d11 -= dt; d22 -= dt; break;
        case 1: dt += dq[2]; d20 += dq[0]; d02 -= dq[0]; d01 += dq[1]; d10 += dq[1]; d12 += dq[3]; d21 += dq[3];
                d00 -= dt; d11 += dt; d22 -= dt; break;
        case 2: dt += dq[3]; d01 += dq[0]; d10 -= dq[0]; d20 += dq[1]; d02 += dq[1]; d12 += dq[2]; d21 += dq[2];
                d00 -= dt; d11 -= dt; d22 += dt; break;
        default: dt += dq[0]; d12 += dq[1]; d21 -= dq[1]; d20 += dq[2]; d02 -= dq[2]; d01 += dq[3]; d10 -= dq[3];
                d00 += dt; d11 += dt; d22 += dt; break;
    }
    // t00 = r[0], t10 = r[1], t20 = r[2], t01 = r[3], t11 = r[4], t21 = r[5], t02 = r[6], t12 = r[7], t22 = r[8]
    dr[0] = d00; dr[1] = d10; dr[2] = d20; dr[3] = d01; dr[4] = d11; dr[5] = d21; dr[6] = d02; dr[7] = d12; dr[8] = d22;
}

// axis-angle -> rotation matrix (row-major R[9]), tgm 0.1.2's angle_axis_to_rotation_matrix: the formula is in eval_metrics.hip's
// head and in include/airpose_grad.h; every fused product is an explicit fmaf (the including files turn contraction off)
__device__ __forceinline__ void aa_to_rotmat(float x, float y, float z, float* R) {
    const float t2 = fmaf(z, z, fmaf(y, y, x * x));
    if (t2 > 1e-6f) {
        const float th = sqrtf(t2);
        const float d = th + 1e-6f;
        const float wx = x / d, wy = y / d, wz = z / d;
        const float c = cosf(th), s = sinf(th);
        const float omc = 1.f - c;
        const float ax = wx * omc, ay = wy * omc, az = wz * omc;
        const float sx = wx * s, sy = wy * s, sz = wz * s;
        R[0] = fmaf(wx, ax, c), R[1] = fmaf(wx, ay, -sz), R[2] = fmaf(wx, az, sy);
        R[3] = fmaf(wx, ay, sz), R[4] = fmaf(wy, ay, c), R[5] = fmaf(wy, az, -sx);
        R[6] = fmaf(wx, az, -sy), R[7] = fmaf(wy, az, sx), R[8] = fmaf(wz, az, c);
    } else {
        R[0] = 1.f, R[1] = -z, R[2] = y;
        R[3] = z, R[4] = 1.f, R[5] = -x;
        R[6] = -y, R[7] = x, R[8] = 1.f;
    }
}
