// normvar's variance-keeping scale (norm.py:248-259) from the one-pass sums, and the rule that says when those sums are not good enough.  Host and device: the
// per-gene solve on the device (csrc/nrm_normvar.hip), the whole-problem entry's host arithmetic (csrc/nrm_host_math.h) and -- restated in numpy -- the Gram-launch
// branch of normalisr_amd/norm.py take the SAME rule, so a gene is marked on every route or on none.
//     dv^2  = s2 / n - mean^2     (the centred variance of the weighted row y' = y e)
//     dv2^2 = (s2 - a . b) / n    (|y' - P y'|^2 = |y'|^2 - a . b)
// Both are differences of fp64 sums: with rho^2 = difference / minuend their relative error is about eps / rho^2, 1e-6 at rho = 1e-5 (a nearly flat row, or one
// that the covariates explain almost completely) and no digit at all below rho = 1e-8, where the clipped difference is 0 and the scale infinite.  A gene with
// either difference below NRM_NV_TAU x its minuend gets NRM_NV_MARK in place of a scale; nrm_normvar_rescale then takes dv and dv2 from the row itself in the
// reference's two-pass form.  Every other gene keeps the value -- and every bit -- of the one-pass form.  wt == 0: the scale is x^0 = 1 whatever x, never marked.
#pragma once
#include <cmath>

#ifndef NRM_HD
#if defined(__HIPCC__)
#define NRM_HD __host__ __device__
#else
#define NRM_HD
#endif
#endif

#define NRM_NV_TAU 0x1p-20  // rho = 2^-10 ~ 1e-3: the one-pass error there is ~ eps / tau = 2.3e-10 ("normvar at kernel level")
#define NRM_NV_MARK (-1.0)  // (a scale is (dv / dv2)^wt >= 0, or NaN: no computed scale is negative)

NRM_HD inline double nrm_nv_scale(double s1, double s2, double ab, double n, double wt) {
	const double mean = s1 / n;
	const double d1 = s2 / n - mean * mean, d2 = s2 - ab;
	if (wt != 0.0 && (d1 < NRM_NV_TAU * (s2 / n) || d2 < NRM_NV_TAU * s2)) return NRM_NV_MARK;
	const double dv = sqrt(fmax(d1, 0.0));       // norm.py:248-249
	const double dv2 = sqrt(fmax(d2, 0.0) / n);  // |y' - P y'|^2 = |y'|^2 - a . b
	return pow(dv / dv2, wt);                    // norm.py:259
}
