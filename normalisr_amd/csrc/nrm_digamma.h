// psi(z), the digamma function, for ONE argument z > 0: what lcpm's table holds at 1 + count and at t0 (lcpm.py:96,101-107 evaluate scipy's digamma there).
// Host and device run the SAME code (csrc/nrm_front_plan.hip: the kernel k_front_tables; tests/host/front_digamma_host.cpp on the CPU), as nrm_fisher.h and
// nrm_jacobi.h do, so that the CPU test-suite can hold it to scipy's values (golden G18: psi_digamma, psi_t0_digamma) without a GPU.
//   z >= 12: the asymptotic series ln z - 1/(2z) - sum_k B_2k / (2k z^2k), k = 1 .. 7; the first term left out is below 2.4e-18.
//   z <  12: shifted upward, psi(z) = psi(z + m) - sum_{i<m} 1/(z + i), with the smallest terms added first; at most 12 terms.
// Every table entry is evaluated on its own: there is no recurrence from one entry to the next, so a thread per entry needs nothing from its neighbours.
// The arithmetic is that of nrm_lcpm_digamma (csrc/nrm_lcpm.hip: lc_psi), which fills the host's table; the two agree to the bar either is held to against scipy.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef NRM_HD
#if defined(__HIPCC__)
#define NRM_HD __host__ __device__
#else
#define NRM_HD
#endif
#endif

#define NRM_DIGAMMA_SHIFT 12.0  // the series is used from here on

NRM_HD inline double nrm_digamma_large(double z) {
	const double w = 1.0 / (z * z);
	double s = 1.0 / 12;  // B_14 / 14
	s = -691.0 / 32760 + w * s;
	s = 1.0 / 132 + w * s;
	s = -1.0 / 240 + w * s;
	s = 1.0 / 252 + w * s;
	s = -1.0 / 120 + w * s;
	s = 1.0 / 12 + w * s;
	return log(z) - 0.5 / z - w * s;
}

NRM_HD inline double nrm_digamma(double z) {
	if (z >= NRM_DIGAMMA_SHIFT) return nrm_digamma_large(z);
	if (!(z > 0.0)) return (z - z) / (z - z);  // lcpm's arguments are positive; anything else (a NaN too) is NaN, and the shift below never runs away
	int m = 0;
	while (z + (double)m < NRM_DIGAMMA_SHIFT) m++;  // (at most 12 for z > 0)
	double shift = 0.0;
	for (int i = m - 1; i >= 0; i--) shift += 1.0 / (z + (double)i);  // the smallest terms first
	return nrm_digamma_large(z + (double)m) - shift;
}
