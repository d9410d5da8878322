// nrm_normvar_host (the expression side of norm.py:166-289) and nrm_binnet_host (binnet.py:134-173), numpy buffers in, numpy buffers out, no torch: the kernels
// normalisr_amd/norm.py and binnet.py drive through the device-pointer entries, with the library's own scratch pool.  normvar's buffers and its launches are the
// step record NrmNormvarStep (nrm_normvar_step.h), which the resident plan of nrm_front_plan.hip runs too; the counters' words are in nrm_front_plan_args.h.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "nrm_front_plan_args.h"
#include "nrm_host_entry.h"
#include "nrm_normvar_step.h"

// ---- binnet (binnet.py:134-173) ------------------------------------------------------------------------------------------------------------
extern "C" int nrm_binnet_host_pk(const void* h_p, int p_dtype, int64_t ng, double qcut, unsigned char* h_net, int64_t* total, int p_kind) {
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(nrm_bind_device());
	NRM_REQUIRE(h_p && h_net && total && ng > 0 && (p_dtype == NRM_F32 || p_dtype == NRM_F64), "nrm_binnet_host: bad arguments");
	NRM_REQUIRE(qcut > 0 && qcut < 1, "qcut must be between 0 and 1.");
	hipStream_t st = nullptr;
	DevBuf dp, dn, tot, flags;
	NRM_TRY(upload_matrix(h_p, p_dtype, ng, ng, dp, st));
	NRM_TRY(dn.alloc((size_t)ng * ng));
	NRM_TRY(tot.alloc_zero(8, st));
	NRM_TRY(flags.alloc_zero(16, st));
	NRM_TRY(nrm_binnet_pk(dp.p, p_dtype, ng, ng, qcut, dn.as<unsigned char>(), ng, tot.as<unsigned long long>(), flags.as<int32_t>(), p_kind, st));
	int32_t hf[4];
	NRM_TRY(nrm_read_flags(flags.p, st, hf));
	if (hf[0]) {
		if (p_kind)
			nrm_set_error("ln P-values must be <= 0 and no NaN: %d rows hold entries that are not", hf[0]);
		else
			nrm_set_error("P-values must be finite and within [0, 1] (binnet.py:151-152): %d rows are not", hf[0]);
		return NRM_E_NUMERIC;
	}
	unsigned long long t = 0;
	NRM_HIP(hipMemcpy(&t, tot.p, 8, hipMemcpyDeviceToHost));
	*total = (int64_t)t;
	return copy_out(h_net, dn.p, (size_t)ng * ng);
}

extern "C" int nrm_binnet_host(const void* h_p, int p_dtype, int64_t ng, double qcut, unsigned char* h_net, int64_t* total) {
	return nrm_binnet_host_pk(h_p, p_dtype, ng, qcut, h_net, total, 0);
}

// ---- normvar (norm.py:166-289): the expression side, whole problem ------------------------------------------------------------------------------
// h_y (rows, n) fp32 / fp64 -> h_out (rows, n): gene g multiplied by e_gk = w_k^wt_g, the covariates C e_g removed, the variance put back (keepvar).  The
// kernels of csrc/nrm_normvar.hip through NrmNormvarStep: solve (per-gene moments in one pass, a lane per gene solving its small OLS with the reference's rank
// rule), then finish (the marked genes' rescale, one pass writing the result).  1 .. nrm_normvar_device_covariates() covariates; up to 32 through the Gram-launch
// form below, which fills the record's b and scale from the host and calls finish
// (NRM_E_UNSUPPORTED beyond: the package's form with numpy's stacked SVD);
// *zero_rank = genes whose covariates have rank 0 (norm.py:158-159 raises for them: the caller does); non-finite results: NRM_E_NUMERIC (norm.py:286).
// The covariates' own scaling (norm.py:261-273) is a few numpy lines on (nc, n) and stays with the caller.
extern "C" int nrm_normvar_host(const void* h_y, int y_dtype, int64_t rows, int64_t n, const double* h_lnw, const double* h_wt, const double* h_c, int64_t nc, double tol,
								int keepvar, void* h_out, int out_dtype, int64_t* zero_rank) {
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(nrm_bind_device());
	NRM_REQUIRE(h_y && h_lnw && h_wt && h_c && h_out && zero_rank && rows > 0 && n > 0 && nc > 0, "nrm_normvar_host: bad arguments");
	NRM_REQUIRE((y_dtype == NRM_F32 || y_dtype == NRM_F64) && (out_dtype == NRM_F32 || out_dtype == NRM_F64), "nrm_normvar_host: bad dtype");
	if (nc > 32) {
		nrm_set_error("nrm_normvar_host: at most 32 covariates (the package's Gram-launch form with numpy's stacked SVD takes more)");
		return NRM_E_UNSUPPORTED;
	}
	hipStream_t st = nullptr;
	DevBuf y, lnw, wt, c, flags, out;
	NRM_TRY(upload_matrix(h_y, y_dtype, rows, n, y, st));
	NRM_TRY(upload_matrix(h_lnw, NRM_F64, 1, n, lnw, st));
	NRM_TRY(upload_matrix(h_wt, NRM_F64, 1, rows, wt, st));
	NRM_TRY(upload_matrix(h_c, NRM_F64, nc, n, c, st));
	NrmNormvarStep nv;
	nv.rows = rows, nv.n = n, nv.ldy = n, nv.nc = nc, nv.ldo = n, nv.tol = tol, nv.keepvar = keepvar, nv.y_dtype = y_dtype, nv.out_dtype = out_dtype;
	nv.d_y = y.p, nv.d_lnw = lnw.as<double>(), nv.d_wt = wt.as<double>(), nv.d_c = c.as<double>();
	const bool wide = nc > nrm_normvar_device_covariates();
	if (wide) {
		// 9 .. 32 covariates (round 6; the entry answered NRM_E_UNSUPPORTED): the Gram-launch form of normalisr_amd/norm.py without torch -- U = e^2 and V = e^2 y
		// (nrm_normvar_weights), M_g = (U P^T)_g with P the nc (nc + 1) / 2 products of covariate rows and a_g = (V C^T)_g on the fp64 Gram kernel, the genes'
		// pseudo-inverses by the library's threaded Jacobi stack (inv_rank's rule: norm.py:152-160), b_g = M_g^+ a_g, the variance-keeping scale (norm.py:248-259),
		// one pass writes the result.
		const int64_t npair = nc * (nc + 1) / 2, rp = nrm_round_up(rows, NRM_ROW_TILE), kp = nrm_round_up(n, NRM_K_TILE), pp = nrm_round_up(npair, NRM_ROW_TILE),
					  cp = nrm_round_up(nc, NRM_ROW_TILE);
		DevBuf u, v, s1, s2, pr, cpad, gm, ga, gwork;
		NRM_TRY(u.alloc((size_t)rp * kp * 8));
		NRM_TRY(v.alloc((size_t)rp * kp * 8));
		NRM_TRY(s1.alloc((size_t)rp * 8));
		NRM_TRY(s2.alloc((size_t)rp * 8));
		NRM_TRY(nrm_normvar_weights(y.p, y_dtype, rows, n, n, lnw.as<double>(), wt.as<double>(), u.as<double>(), v.as<double>(), kp, rp, s1.as<double>(), s2.as<double>(), st));
		{  // the operands of the two contractions, built on the host from the covariates (a few MB)
			const double* hc = h_c;
			std::vector<double> hp((size_t)pp * kp, 0.0), hcp((size_t)cp * kp, 0.0);
			int64_t j = 0;
			for (int64_t a = 0; a < nc; a++)
				for (int64_t d = a; d < nc; d++, j++)
					for (int64_t k = 0; k < n; k++) hp[(size_t)(j * kp + k)] = hc[a * n + k] * hc[d * n + k];
			for (int64_t a = 0; a < nc; a++) memcpy(&hcp[(size_t)(a * kp)], hc + a * n, (size_t)n * 8);
			NRM_TRY(pr.alloc(hp.size() * 8));
			NRM_TRY(cpad.alloc(hcp.size() * 8));
			NRM_HIP(hipMemcpy(pr.p, hp.data(), hp.size() * 8, hipMemcpyHostToDevice));
			NRM_HIP(hipMemcpy(cpad.p, hcp.data(), hcp.size() * 8, hipMemcpyHostToDevice));
		}
		NRM_TRY(gm.alloc((size_t)rp * pp * 8));
		NRM_TRY(ga.alloc((size_t)rp * cp * 8));
		NRM_TRY(gwork.alloc((size_t)nrm_gram_workspace_bytes()));
		NRM_TRY(nrm_gram_f64(u.as<double>(), pr.as<double>(), rp, pp, kp, kp, kp, gm.as<double>(), pp, 0, rows, npair, gwork.p, st));
		NRM_TRY(nrm_gram_f64(v.as<double>(), cpad.as<double>(), rp, cp, kp, kp, kp, ga.as<double>(), cp, 0, rows, nc, gwork.p, st));
		std::vector<double> hgm, hga, hs1, hs2;
		NRM_TRY(download(hgm, gm.p, (size_t)rp * pp));
		NRM_TRY(download(hga, ga.p, (size_t)rp * cp));
		NRM_TRY(download(hs1, s1.p, (size_t)rows));
		NRM_TRY(download(hs2, s2.p, (size_t)rows));
		u.release();
		v.release();
		std::vector<double> m((size_t)rows * nc * nc), mi((size_t)rows * nc * nc), hb, hscale;
		std::vector<int64_t> rk((size_t)rows, 0);
		for (int64_t g = 0; g < rows; g++) {
			int64_t j = 0;
			for (int64_t a = 0; a < nc; a++)
				for (int64_t d = a; d < nc; d++, j++) m[(size_t)((g * nc + a) * nc + d)] = m[(size_t)((g * nc + d) * nc + a)] = hgm[(size_t)(g * pp + j)];
		}
		NRM_TRY(nrm_small_pinv(m.data(), rows, nc, tol, mi.data(), rk.data(), 0));
		int64_t zr = 0;
		for (int64_t g = 0; g < rows; g++) zr += rk[(size_t)g] <= 0;
		*zero_rank = zr;
		if (zr) return NRM_OK;
		nrm_normvar_coefficients(mi.data(), hga.data(), cp, hs1.data(), hs2.data(), h_wt, rows, nc, n, keepvar, hb, hscale);
		NRM_TRY(nv.alloc_coefficients(nrm_take_plain));
		NRM_HIP(hipMemcpy(nv.b.p, hb.data(), hb.size() * 8, hipMemcpyHostToDevice));
		NRM_HIP(hipMemcpy(nv.scale.p, hscale.data(), hscale.size() * 8, hipMemcpyHostToDevice));
		NRM_TRY(flags.alloc_zero(16, st));
		nv.flags = flags.as<int32_t>();
	} else {
		NRM_TRY(nv.alloc(nrm_take_plain));
		NRM_TRY(flags.alloc_zero(16, st));
		nv.flags = flags.as<int32_t>();
		NRM_TRY(nv.solve(st));
	}
	// the rescale of the genes either route has marked, then the one pass that writes the result from b_g and the scale: NrmNormvarStep::finish
	const size_t ob = (size_t)rows * n * nrm_esize(out_dtype);
	NRM_TRY(out.alloc(ob));
	nv.d_out = out.p;
	NRM_TRY(nv.finish(st));
	int32_t hf[4];
	NRM_TRY(nrm_read_flags(flags.p, st, hf));
	if (!wide) {
		*zero_rank = hf[0];
		if (hf[0]) return NRM_OK;
	}
	const int32_t results[2] = {0, hf[1]};  // (rank 0 is the caller's to raise, from *zero_rank)
	NRM_TRY(nrm_normvar_status(results));
	return copy_out(h_out, out.p, ob);
}
