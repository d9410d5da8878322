"""The child side of tests/test_gpu_bh.py: `normalisr bh pv_in q_out` in a process in which torch cannot be imported (as tests/coex_plan_child.py).
`python tests/bh_cli_child.py PV_IN Q_OUT [PV_IN Q_OUT ...]`."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
	sys.modules['torch'] = None  # `import torch` raises ImportError in this process
	sys.path.insert(0, ROOT)
	from normalisr_amd.__main__ import main as normalisr
	for src, dst in zip(argv[1::2], argv[2::2]):
		assert normalisr(['bh', src, dst]) == 0
	assert sys.modules['torch'] is None and not [m for m in sys.modules if m.startswith('torch.')]
	print('child ok')


if __name__ == '__main__':
	main(sys.argv)
