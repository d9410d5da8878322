"""The folded schedule of the integer Gram kernel on the CPU: csrc/nrm_host_logic.h (gram_plan_fold, gram_sched_coords) built by g++ with
-fsanitize=address,undefined and run by a stand-alone program (tests/host/fold_sanitize.cpp)."""
from cabi_harness import build_and_run_host_program


def test_integer_gram_fold_schedule_under_address_and_ub_sanitizers(tmp_path):
	"""A symmetric whole-matrix launch whose last tile column holds 1 to 32 valid columns lists the leading grid's upper triangle and the corner
	tile only; diagonal tiles host the last column's tiles.  For tile grids of 2 to 45 columns, 8 to 512 workgroups and 1 to 400 k-units: every
	k-unit of every listed tile is covered exactly once, no off-diagonal tile of the last column is listed, every host diagonal tile is, every slab
	lies inside the workspace; launches the fold does not apply to keep gram_plan's schedule field for field."""
	build_and_run_host_program(tmp_path, ['tests/host/fold_sanitize.cpp'], 'fold schedule ok', may_skip=True)
