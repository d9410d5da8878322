// nrm_jacobi.h's pseudo-inverse of ONE symmetric matrix with the work of a rotation spread over cooperating lanes: the same cyclic sequence of rotations
// (p, q), the same arithmetic per element -- the three k-loops of a rotation touch independent elements, lane l takes k = l, l + lanes, ... -- and the rank
// rule of inv_rank (association.py:77-80).  a and v live where every lane sees them (LDS on the device: 2 x 63^2 doubles fit below 64 KB), so no lane
// keeps an n x n array of its own.  X says who the lanes are: NrmSerialLanes (one lane, the host twin nrm_fitvar_pinv_host and the CPU tests) or a workgroup
// (csrc/nrm_fitvar_plan.hip).  Every branch below depends on shared values only, so all lanes reach every sync().
#pragma once
#include "nrm_jacobi.h"

struct NrmSerialLanes {
	NRM_HD int lane() const { return 0; }
	NRM_HD int lanes() const { return 1; }
	NRM_HD void sync() const {}
};

// a (n x n, row-major, symmetric, visible to every lane before the call; destroyed), v (n x n), w (n), red (2 n): shared scratch.
// inv (n x n) = the pseudo-inverse, *rank = the number of eigenvalues kept (written by lane 0).
template <class X>
NRM_HD inline void nrm_pinv_lanes(const X& x, double* a, double* v, double* w, double* red, int n, double tol, double* inv, int64_t* rank) {
	const int lane = x.lane(), nl = x.lanes();
	for (int i = lane; i < n * n; i += nl) v[i] = i / n == i % n ? 1.0 : 0.0;
	x.sync();
	for (int sweep = 0; sweep < 60; sweep++) {
		for (int i = lane; i < n; i += nl) {  // a row's share of the two sums each, the rows then added in order by everybody
			double o = 0.0;
			for (int j = i + 1; j < n; j++) o += a[i * n + j] * a[i * n + j];
			red[i] = o;
			red[n + i] = a[i * n + i] * a[i * n + i];
		}
		x.sync();
		double off = 0.0, diag = 0.0;
		for (int i = 0; i < n; i++) off += red[i], diag += red[n + i];
		x.sync();
		if (off == 0.0 || off <= 1e-34 * diag) break;
		for (int p = 0; p < n - 1; p++)
			for (int q = p + 1; q < n; q++) {
				const double apq = a[p * n + q];
				if (apq == 0.0) continue;
				const double theta = (a[q * n + q] - a[p * n + p]) / (2.0 * apq);
				const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
				const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
				x.sync();  // (everybody has read a_pq, a_pp, a_qq)
				for (int k = lane; k < n; k += nl) {  // columns p, q
					const double akp = a[k * n + p], akq = a[k * n + q];
					a[k * n + p] = c * akp - s * akq;
					a[k * n + q] = s * akp + c * akq;
				}
				x.sync();
				for (int k = lane; k < n; k += nl) {  // rows p, q (a_pq = a_qp = 0 exactly, as nrm_jacobi sets them), and the eigenvectors
					const double apk = a[p * n + k], aqk = a[q * n + k];
					a[p * n + k] = k == q ? 0.0 : c * apk - s * aqk;
					a[q * n + k] = k == p ? 0.0 : s * apk + c * aqk;
					const double vkp = v[k * n + p], vkq = v[k * n + q];
					v[k * n + p] = c * vkp - s * vkq;
					v[k * n + q] = s * vkp + c * vkq;
				}
				x.sync();
			}
	}
	for (int i = lane; i < n; i += nl) w[i] = a[i * n + i];
	x.sync();
	double smax = 0.0;
	for (int i = 0; i < n; i++) smax = fmax(smax, fabs(w[i]));
	int r = 0;
	for (int i = 0; i < n; i++) r += fabs(w[i]) >= tol * smax;  // (a zero matrix keeps everything and divides by zero, as the reference does)
	for (int i = lane; i < n; i += nl) red[i] = fabs(w[i]) >= tol * smax ? 1.0 / w[i] : 0.0;
	x.sync();
	for (int e = lane; e < n * n; e += nl) {
		const int i = e / n, j = e % n;
		if (j > i) continue;
		double t = 0.0;
		for (int k = 0; k < n; k++)
			if (red[k] != 0.0) t += v[i * n + k] * red[k] * v[j * n + k];
		inv[i * n + j] = inv[j * n + i] = t;
	}
	if (lane == 0) *rank = r;
}
