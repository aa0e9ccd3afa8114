"""Unit coverage of class M's row-mask path (csrc/dcr_bfc_h2.hip, h2_rows_unit) on the bench graphs, on the GPU box:

    python tools/h2_rowmask_coverage.py [--nodes 100000 1000000]

One forced two-hop pass per graph; prints the class-M units of the pass, how many of them the row-mask path published and how many
it handed over to the block path (the library's diagnostic counter, dcr_h2_rowmask_units, which is not part of h2_stats())."""
import argparse
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'discrete-curvature-rewiring_amd')]
os.environ['DCR_PASS'] = 'h2'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, nargs='+', default=[100000, 1000000])
    args = ap.parse_args()
    from dcr import _lib, synthetic
    from dcr.graph import DcrGraph
    fn = _lib.lib().dcr_h2_rowmask_units
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_uint32)]
    out = (ctypes.c_uint32 * 2)()
    for nodes in args.nodes:
        ei, n = synthetic.powerlaw_graph(nodes, 10, seed=12345)
        G = DcrGraph(ei, n)
        G.curvature_all('bfc')              # (the first pass of a graph may be launched twice: the counted one follows)
        assert fn(out) == 0
        G.curvature_all('bfc')
        assert fn(out) == 0
        stats, info = G.h2_stats(), G.h2_launch_info()
        assert G.pass_engine() == 'two-hop' and info['launches'] == 1, info
        m = stats['units_m']
        print('N=%d: class-M units %d, row-mask path published %d (%.1f %%), handed over %d (%.2f %%), block path %d; retry %d fallback %d'
              % (n, m, out[0], 100.0 * out[0] / max(m, 1), out[1], 100.0 * out[1] / max(m, 1), m - out[0], stats['retry'], stats['fallback']))
        G.close()


if __name__ == '__main__':
    main()
