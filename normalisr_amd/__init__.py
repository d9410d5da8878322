"""normalisr_amd: MI355X-native implementation of Normalisr's linear-association hot path
(norm.de / norm.coex).  Importing submodules mirrors the reference package layout:
normalisr_amd.normalisr, .de, .coex, .association, .parallel, .run, .qc, .gocovt; .enrich, .levels and .cplan (resident coex through the C ABI's plan handle: numpy and ctypes only) are this build's own."""
__all__ = ['association', 'binnet', 'coex', 'cplan', 'de', 'enrich', 'gocovt', 'levels', 'norm', 'normalisr', 'parallel', 'qc', 'run']
__version__ = '0.1.0'
