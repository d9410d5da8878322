"""The child side of tests/test_gpu_single1_wide.py: a process in which torch cannot be imported calls nrm_association_tests_single1_host (through
normalisr_amd.association._single14_host_entry: numpy buffers in and out) on the arrays of IN.npz and writes what came back.
`python tests/single1_wide_child.py IN.npz OUT.npz`; the entry's own trace lines (NRM_DEBUG=s1_trace=1) go to stderr, which the parent reads."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('p', 'gamma', 'alpha', 'varx', 'vary')


def main(argv):
	sys.modules['torch'] = None  # `import torch` raises ImportError in this process
	sys.path.insert(0, ROOT)
	from normalisr_amd import association
	arr = np.load(argv[1])
	res = association._single14_host_entry(1, arr['dx'], arr['dy'], arr['dc'], False, False, {})
	assert sys.modules['torch'] is None and not [m for m in sys.modules if m.startswith('torch.')]
	np.savez(argv[2], **dict(zip(KEYS, res)))
	print('child ok')


if __name__ == '__main__':
	main(sys.argv)
