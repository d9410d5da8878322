"""The folded schedule of the integer Gram kernel on the CPU: csrc/nrm_host_logic.h (gram_plan_fold, gram_sched_coords) built by g++ with
-fsanitize=address,undefined and run by a stand-alone program (tests/host/fold_sanitize.cpp)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_integer_gram_fold_schedule_under_address_and_ub_sanitizers(tmp_path):
	"""A symmetric whole-matrix launch whose last tile column holds 1 to 32 valid columns lists the leading grid's upper triangle and the corner
	tile only; diagonal tiles host the last column's tiles.  For tile grids of 2 to 45 columns, 8 to 512 workgroups and 1 to 400 k-units: every
	k-unit of every listed tile is covered exactly once, no off-diagonal tile of the last column is listed, every host diagonal tile is, every slab
	lies inside the workspace; launches the fold does not apply to keep gram_plan's schedule field for field."""
	gxx = shutil.which('g++')
	if gxx is None:
		pytest.skip('no g++')
	flags = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
	# whether the sanitizer runtimes are installed is decided on a one-line program: a failed build of the real source is a failure, never a skip
	probe = tmp_path / 'probe.cpp'
	probe.write_text('int main() { return 0; }\n')
	r = subprocess.run([gxx] + flags + ['-o', str(tmp_path / 'probe'), str(probe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
	if r.returncode != 0:
		pytest.skip('g++ cannot build with -fsanitize=address,undefined here: ' + r.stdout[-200:])
	exe = str(tmp_path / 'fold_check')
	src = os.path.join(ROOT, 'tests', 'host', 'fold_sanitize.cpp')
	r = subprocess.run([gxx] + flags + ['-o', exe, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
	assert r.returncode == 0, r.stdout[-3000:]
	r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
	assert r.returncode == 0 and 'fold schedule ok' in r.stdout, r.stdout[-2000:]
