// cpe_detection.hip.inc -- the detection report (include/cpe.h, cpe_detection_report; DESIGN.md 2 "What is predicted in the image"): every
// marker's predicted pixel in every camera with its 2 x 2 covariance S = G Sigma_p G^T and, where there are detections, the prediction with
// that one detection left out of the fit (Woodbury on its 2 x 2 term of H: no second factorisation), its covariance, the chi-square distance of
// the detection from it and the detection's share of the hat matrix's trace.
//
// One wave per frame, lanes stride over the (camera, marker) pairs as k_reproject's do; registers only, no LDS, no atomics: every output entry
// is a function of its own pair's inputs alone, so a frame's outputs do not depend on the launch it is part of.  uv is k_reproject's
// arithmetic: the same project_point on the handle's camera.  MEAS = false is the pixel-ellipse part alone (meas, weight, weight_fit and the
// four outputs after cov_px are not touched).  Each of those four outputs may be null on its own.

// the 2 x 2 symmetric product B M B^T as (xx, xy, yy); B general, M symmetric (m00, m01, m11)
__device__ __forceinline__ void det_congruence(double b00, double b01, double b10, double b11, double m00, double m01, double m11,
                                               double& xx, double& xy, double& yy) {
    const double c00 = b00 * m00 + b01 * m01, c01 = b00 * m01 + b01 * m11;
    const double c10 = b10 * m00 + b11 * m01, c11 = b10 * m01 + b11 * m11;
    xx = c00 * b00 + c01 * b01;
    xy = c00 * b10 + c01 * b11;
    yy = c10 * b10 + c11 * b11;
}

template <bool MEAS>
__global__ __launch_bounds__(WAVE) void k_detection_report(const DevModel* __restrict__ M, const double* __restrict__ positions,
                                                           const double* __restrict__ cov_pos, const double* __restrict__ meas,
                                                           const double* __restrict__ weight, const double* __restrict__ weight_fit,
                                                           double* __restrict__ uv, double* __restrict__ cov_px, double* __restrict__ uv_loo,
                                                           double* __restrict__ cov_loo, double* __restrict__ d2, double* __restrict__ leverage) {
    const int L = M->L, CL = M->C * L;
    const size_t f = blockIdx.x;
    const double* P = positions + f * (size_t)(3 * L);
    const double* SP = cov_pos + f * (size_t)(9 * L);
    const double la = M->loss_a, lb = M->loss_b, lc = M->loss_c;
    const int mode = M->curvature;
    const double nan = __builtin_nan("");
    // curvature of the loss at its centre: the Gaussian the loss is there has variance 1 / (w^2 kappa0)
    const double kappa0 = MEAS ? robust_loss(0.0, la, lb, lc, mode, true).cw : 0.0;
    for (int t = threadIdx.x; t < CL; t += WAVE) {
        const int c = t / L, l = t - c * L;
        const size_t o = f * (size_t)CL + t;
        double u, v, G[6];
        project_point(M->cam[c], P[3 * l], P[3 * l + 1], P[3 * l + 2], u, v, G);
        reinterpret_cast<double2*>(uv)[o] = make_double2(u, v);
        // S = G Sigma_p G^T
        const double* Sg = SP + 9 * l;
        double A0[3], A1[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            A0[j] = G[0] * Sg[j] + G[1] * Sg[3 + j] + G[2] * Sg[6 + j];
            A1[j] = G[3] * Sg[j] + G[4] * Sg[3 + j] + G[5] * Sg[6 + j];
        }
        const double s00 = A0[0] * G[0] + A0[1] * G[1] + A0[2] * G[2];
        const double s01 = A0[0] * G[3] + A0[1] * G[4] + A0[2] * G[5];
        const double s11 = A1[0] * G[3] + A1[1] * G[4] + A1[2] * G[5];
        cov_px[3 * o] = s00; cov_px[3 * o + 1] = s01; cov_px[3 * o + 2] = s11;
        if (!MEAS) continue;

        const double2 z = reinterpret_cast<const double2*>(meas)[o];
        const double mult = M->cam[c].mult;
        const double w = mult * weight[o], wf = mult * weight_fit[o];
        double ul = u, vl = v, l00 = s00, l01 = s01, l11 = s11, dist = nan, lev = 0.0;
        if (w != 0.0) {
            // the gradient and curvature terms this detection put into H (k_frame_normal's)
            const LossOut q0 = robust_loss(wf * (u - z.x), la, lb, lc, mode, true);
            const LossOut q1 = robust_loss(wf * (v - z.y), la, lb, lc, mode, true);
            const double g0 = q0.d1 * wf, g1 = q1.d1 * wf;
            const double W0 = q0.cw * wf * wf, W1 = q1.cw * wf * wf;
            const double a0 = sqrt(W0), a1 = sqrt(W1);
            lev = W0 * s00 + W1 * s11;
            // T = I - diag(a) S diag(a) and its smaller eigenvalue
            const double t00 = 1.0 - a0 * s00 * a0, t01 = -(a0 * s01 * a1), t11 = 1.0 - a1 * s11 * a1;
            const double hd = 0.5 * (t00 - t11);
            const double lmin = 0.5 * (t00 + t11) - sqrt(hd * hd + t01 * t01);
            if (lmin > 1e-9 && fabs(lmin) != INFINITY) {            // (a NaN fails the comparison)
                // S_loo = S + (S diag a) T^-1 (S diag a)^T
                const double idet = 1.0 / (t00 * t11 - t01 * t01);
                double xx, xy, yy;
                det_congruence(s00 * a0, s01 * a1, s01 * a0, s11 * a1, t11 * idet, -t01 * idet, t00 * idet, xx, xy, yy);
                l00 = s00 + xx; l01 = s01 + xy; l11 = s11 + yy;
                ul = u + (l00 * g0 + l01 * g1);
                vl = v + (l01 * g0 + l11 * g1);
                // d2 = r^T (S_loo + sigma2 I)^-1 r,  r = z - uv_loo
                const double sigma2 = 1.0 / (w * w * kappa0);
                const double c00 = l00 + sigma2, c11 = l11 + sigma2;
                const double r0 = z.x - ul, r1 = z.y - vl;
                dist = (c11 * r0 * r0 - 2.0 * l01 * r0 * r1 + c00 * r1 * r1) / (c00 * c11 - l01 * l01);
            } else {
                ul = vl = l00 = l01 = l11 = nan;        // the detection alone determines a direction: nothing is left to predict it from
            }
        }
        if (uv_loo) reinterpret_cast<double2*>(uv_loo)[o] = make_double2(ul, vl);
        if (cov_loo) { cov_loo[3 * o] = l00; cov_loo[3 * o + 1] = l01; cov_loo[3 * o + 2] = l11; }
        if (d2) d2[o] = dist;
        if (leverage) leverage[o] = lev;
    }
}
