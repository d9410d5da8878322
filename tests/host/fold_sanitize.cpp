// CPU build of the folded Gram schedule (csrc/nrm_host_logic.h: gram_plan_fold, gram_sched_coords) for g++ -fsanitize=address,undefined
// (tests/test_gram_fold_cpu.py builds and runs it).  A symmetric launch over the whole matrix whose last tile column holds 1 to 32 valid
// columns lists the upper triangle of the leading (ntn - 1) x (ntn - 1) grid and the corner tile; the off-diagonal tiles of the last column
// ride in the diagonal tiles (their hosts).  For tile grids of 2 to 45 columns, 8 to 512 workgroups and 1 to 400 k-units this checks that
//  * every k-unit of every listed tile is covered exactly once by the pieces of the workgroups;
//  * no off-diagonal tile of the last column is listed, every host diagonal tile and the corner tile are, no tile twice;
//  * every slab lies inside the workspace and nobody shares one;
//  * launches the fold does not apply to (0 or more than 32 valid columns, bands, rectangular, one tile column) get gram_plan's schedule.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include "../../normalisr_amd/csrc/nrm_host_logic.h"

static char g_err[512];
void nrm_set_error(const char* fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
}

#define CHECK(c)                                                              \
	do {                                                                      \
		if (!(c)) {                                                           \
			fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
			exit(1);                                                          \
		}                                                                     \
	} while (0)

static bool same_schedule(const GramSched& a, const GramSched& b) {
	return a.m_rows == b.m_rows && a.n_rows == b.n_rows && a.ntm == b.ntm && a.ntn == b.ntn && a.nkt == b.nkt && a.tiles_dp == b.tiles_dp &&
		   a.tiles_al == b.tiles_al && a.parts == b.parts && a.tiles_sk == b.tiles_sk && a.units_per_wg == b.units_per_wg && a.nwg == b.nwg &&
		   a.tile0 == b.tile0 && a.accumulate == b.accumulate && a.fold == b.fold && a.work == b.work;
}

static long g_folded = 0;
static double* g_work = nullptr;  // a workspace of the largest launch checked, never touched: slab pointers are formed inside an object that exists
static const int kMaxWg = 512;

static void check_folded(int ntn, int valid, int64_t nkt, int nwg) {
	const int64_t pad = (int64_t)ntn * GN, rows = (int64_t)(ntn - 1) * GN + valid;
	GramSched s;
	CHECK(nwg <= kMaxWg);
	CHECK(gram_plan_fold(s, pad, pad, nkt, 1, rows, rows, 0, pad, nwg, g_work) == NRM_OK);
	CHECK(s.fold == ntn - 1 && s.tile0 == 0 && s.accumulate == 0 && s.nwg == nwg - nwg % 8);
	const int lead = ntn - 1, tiles = s.tiles_dp + s.tiles_al + s.tiles_sk;
	CHECK(tiles == lead * (lead + 1) / 2 + 1);
	CHECK(s.tiles_al * s.parts <= s.nwg);
	// the tile list
	std::set<std::pair<int, int>> listed;
	for (int t = 0; t < tiles; t++) {
		int ti = -1, tj = -1;
		gram_sched_coords(s, t, 1, ti, tj);
		CHECK(ti >= 0 && ti <= tj && tj < ntn);
		CHECK(tj < lead || ti == lead);  // no off-diagonal tile of the last column
		CHECK(listed.insert({ti, tj}).second);
		CHECK(gram_is_host(s, ti, tj) == (ti == tj && ti < lead));
	}
	for (int i = 0; i < ntn; i++) CHECK(listed.count({i, i}) == 1);  // every host and the corner
	for (int i = 0; i < lead; i++)
		for (int j = i; j < lead; j++) CHECK(listed.count({i, j}) == 1);
	// the pieces
	std::vector<std::vector<int>> cover((size_t)tiles, std::vector<int>((size_t)nkt, 0));
	std::set<const double*> slabs;
	for (int b = 0; b < s.nwg; b++)
		gram_pieces_of(s, b, [&](int t, int k0, int k1, double* slab) {
			CHECK(t >= 0 && t < tiles && k0 >= 0 && k0 < k1 && k1 <= nkt);
			for (int k = k0; k < k1; k++) cover[(size_t)t][(size_t)k]++;
			if (slab) {
				CHECK(slab >= g_work && (int64_t)(slab - g_work) + GM * GN <= nrm_host_gram_workspace_doubles(s.nwg));
				CHECK(slabs.insert(slab).second);
			} else
				CHECK(k0 == 0 && k1 == nkt);
		});
	for (int t = 0; t < tiles; t++)
		for (int64_t k = 0; k < nkt; k++) CHECK(cover[(size_t)t][(size_t)k] == 1);
	g_folded++;
}

static void check_not_folded(int64_t m_pad, int64_t n_pad, int64_t nkt, int symmetric, int64_t m_rows, int64_t n_rows, int64_t row0, int64_t row1, int nwg) {
	GramSched a, b;
	CHECK(gram_plan(a, m_pad, n_pad, nkt, symmetric, m_rows, n_rows, row0, row1, nwg, g_work) == NRM_OK);
	CHECK(gram_plan_fold(b, m_pad, n_pad, nkt, symmetric, m_rows, n_rows, row0, row1, nwg, g_work) == NRM_OK);
	CHECK(a.fold == 0 && same_schedule(a, b));
	for (int t = 0; t < a.tiles_dp + a.tiles_al + a.tiles_sk && t < 2000; t++) {
		int ti, tj, ui, uj;
		gram_tile_coords(a.tile0 + t, symmetric, a.ntm, a.ntn, ti, tj);
		gram_sched_coords(b, t, symmetric, ui, uj);
		CHECK(ti == ui && tj == uj && !gram_is_host(b, ui, uj));
	}
}

int main() {
	g_work = (double*)malloc((size_t)nrm_host_gram_workspace_doubles(kMaxWg) * sizeof(double));
	CHECK(g_work != nullptr);
	const int nwgs[] = {8, 16, 64, 104, 256, 304, 512};
	const int64_t nkts[] = {1, 2, 3, 7, 8, 15, 16, 31, 32, 63, 64, 65, 100, 313, 400};
	for (int ntn = 2; ntn <= 45; ntn++)
		for (int nwg : nwgs)
			for (int64_t nkt : nkts) check_folded(ntn, (ntn * 7 + nwg) % 32 + 1, nkt, nwg);
	for (int valid : {1, 8, 31, 32}) {
		check_folded(40, valid, 313, 256);  // 5000 genes x 10 000 cells: 781 tiles
		check_folded(2, valid, 3, 256);
	}
	{
		GramSched s;
		CHECK(gram_plan_fold(s, 5120, 5120, 313, 1, 5000, 5000, 0, 5120, 256, g_work) == NRM_OK);
		CHECK(s.fold == 39 && s.tiles_dp + s.tiles_al + s.tiles_sk == 781);
	}
	// where the fold does not apply
	for (int nwg : {8, 256, 304})
		for (int64_t nkt : {3, 64, 313}) {
			check_not_folded(5120, 5120, nkt, 1, 5025, 5025, 0, 5120, nwg);  // 33 valid columns
			check_not_folded(5120, 5120, nkt, 1, 0, 0, 0, 5120, nwg);        // a full last column
			check_not_folded(5120, 5120, nkt, 1, 5120, 5120, 0, 5120, nwg);
			check_not_folded(5120, 5120, nkt, 1, 4992, 4992, 0, 5120, nwg);  // 0 valid columns in the last one
			check_not_folded(128, 128, nkt, 1, 8, 8, 0, 128, nwg);           // one tile column
			check_not_folded(5120, 5120, nkt, 0, 5000, 5000, 0, 5120, nwg);  // not symmetric
			check_not_folded(1024, 5120, nkt, 0, 1000, 5000, 0, 1024, nwg);  // rectangular
			check_not_folded(5120, 5120, nkt, 1, 5000, 5000, 0, 1024, nwg);  // bands
			check_not_folded(5120, 5120, nkt, 1, 5000, 5000, 4096, 5120, nwg);
		}
	CHECK(g_folded > 4000);
	free(g_work);
	printf("fold schedule ok (%ld folded schedules)\n", g_folded);
	return 0;
}
