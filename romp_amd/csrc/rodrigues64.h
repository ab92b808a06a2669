// rodrigues64.h -- the SMPL layer's Rodrigues formula (smpl.py:191-222, the 1e-8 of :206 included) and its derivative in
// float64, as smpl_grad_person_kernel (smpl_grad.hip) differentiates it: R = I + sin K(d) + (1 - cos) K(d)^2, d = rv / angle,
// angle = |rv + 1e-8|.  For kernels that need a joint's rotation matrix and the gradient of a function of it.
#pragma once
#include <math.h>

namespace romp {

struct Rodrigues64 { double rv[3], ev[3], angle, sn, cs, K[9], K2[9]; };

// rv: three float32 axis-angle columns -> R (row-major 3x3); `s` keeps what the backward needs
__device__ __forceinline__ void rodrigues64(const float* rv, double (&R)[9], Rodrigues64& s) {
    for (int k = 0; k < 3; ++k) {
        s.rv[k] = (double)rv[k];
        s.ev[k] = s.rv[k] + 1e-8;
    }
    s.angle = sqrt(s.ev[0] * s.ev[0] + s.ev[1] * s.ev[1] + s.ev[2] * s.ev[2]);
    const double dx = s.rv[0] / s.angle, dy = s.rv[1] / s.angle, dz = s.rv[2] / s.angle;
    sincos(s.angle, &s.sn, &s.cs);
    double* K = s.K;
    K[0] = 0; K[1] = -dz; K[2] = dy; K[3] = dz; K[4] = 0; K[5] = -dx; K[6] = -dy; K[7] = dx; K[8] = 0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) s.K2[r * 3 + c] = K[r * 3] * K[c] + K[r * 3 + 1] * K[3 + c] + K[r * 3 + 2] * K[6 + c];
    for (int e = 0; e < 9; ++e) R[e] = ((e == 0 || e == 4 || e == 8) ? 1.0 : 0.0) + s.sn * K[e] + (1.0 - s.cs) * s.K2[e];
}

// gR = d f / d R  ->  g = d f / d rv
__device__ __forceinline__ void rodrigues64_backward(const Rodrigues64& s, const double (&gR)[9], double (&g)[3]) {
    const double* K = s.K;
    double gs = 0, goc = 0;
    for (int e = 0; e < 9; ++e) { gs += gR[e] * K[e]; goc += gR[e] * s.K2[e]; }
    double gang = s.cs * gs + s.sn * goc;
    double gK[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double t = 0;                                         // (G K^T + K^T G)[r][c]
            for (int k = 0; k < 3; ++k) t += gR[r * 3 + k] * K[c * 3 + k] + K[k * 3 + r] * gR[k * 3 + c];
            gK[r * 3 + c] = s.sn * gR[r * 3 + c] + (1.0 - s.cs) * t;
        }
    const double gd[3] = {gK[7] - gK[5], gK[2] - gK[6], gK[3] - gK[1]};
    gang -= (gd[0] * s.rv[0] + gd[1] * s.rv[1] + gd[2] * s.rv[2]) / (s.angle * s.angle);
    for (int k = 0; k < 3; ++k) g[k] = gd[k] / s.angle + gang * s.ev[k] / s.angle;
}

}  // namespace romp
