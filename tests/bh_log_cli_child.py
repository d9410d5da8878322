"""The child side of tests/test_gpu_bh_log.py and tests/test_gpu_binnet_log.py: `normalisr bh pv_in q_out --logp` and `normalisr binnet pv_in net_out qcut --logp`
in a process in which torch cannot be imported (as tests/bh_cli_child.py).
`python tests/bh_log_cli_child.py CMD IN OUT QCUT [CMD IN OUT QCUT ...]`, CMD one of bh, binnet; QCUT is '-' for bh."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
	sys.modules['torch'] = None  # `import torch` raises ImportError in this process
	sys.path.insert(0, ROOT)
	from normalisr_amd.__main__ import main as normalisr
	a = argv[1:]
	for cmd, src, dst, qcut in zip(a[0::4], a[1::4], a[2::4], a[3::4]):
		assert normalisr([cmd, src, dst, '--logp'] if cmd == 'bh' else [cmd, src, dst, qcut, '--logp']) == 0
	assert sys.modules['torch'] is None and not [m for m in sys.modules if m.startswith('torch.')]
	print('child ok')


if __name__ == '__main__':
	main(sys.argv)
