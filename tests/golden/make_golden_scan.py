"""Golden fixture for the all-pairs scans of the cluster and the manifold stage: runs the cases of tests/scan_cases.py through the
library as it is built in this tree, on the GPU, and stores the shape and the SHA-256 of every output's bytes in ref_scan.json;
for the smallest cases of each stage the arrays themselves too (a float's JSON form reads back to the same bits), so a mismatch
can be read.  Both stages are deterministic, so the fixture pins their bytes.

It was run once, on an MI355X at the commit before both stages' scans were put on csrc/nm_scan.h, and is not run again to make a
failing test pass: a refactor that changes a byte is wrong.

    python tests/golden/make_golden_scan.py"""
import json
import os
import sys

import numpy as np

os.environ['PYTHONDONTWRITEBYTECODE'] = '1'
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
import scan_cases as S  # noqa: E402

READABLE = {S.cluster_key(1, 1), S.cluster_key(255, 1), S.affinity_key(127, 1), S.gradient_key(129, 1)}


def entry(key, out):
    e = {'outputs': {name: S.digest(a) for name, a in out.items()}}
    if key in READABLE:
        e['arrays'] = {name: a.tolist() for name, a in out.items()}
    return e


def main():
    cases = {}
    for nd in S.CL_ND:
        for n in S.CL_N:
            out = S.cluster_case(n, nd)
            label, core = out['label'], out['degree'] >= S.CL_MIN_PTS
            if n >= 255:
                assert core.any() and (~core & (label >= 0)).any() and (label < 0).any(), (n, nd)
            cases[S.cluster_key(n, nd)] = entry(S.cluster_key(n, nd), out)
    lists = {}
    for nd in S.AF_ND:
        for n in S.AF_N:
            rc, msg, out = S.affinity_call(n, nd)
            key = S.affinity_key(n, nd)
            if n == 3:                                              # k = 2 admits no perplexity k / 3 in (1, k)
                assert rc == S.B.NM_ERR_ARG and all((a == -77).all() for a in out.values()), (rc, msg)
                cases[key] = {'rc': rc, 'message': msg}
                continue
            assert rc == S.B.NM_OK, msg
            assert (out['nbr'] >= 0).all() and np.isfinite(out['p']).all() and (out['beta'] > 0).all()
            cases[key] = entry(key, out)
            lists[n, nd] = out
    for nc in S.GR_NC:
        for n in S.GR_N:
            out = S.gradient_case(n, nc, lists[n, S.AF_ND[-1]])
            assert all(np.isfinite(a).all() for a in out.values()) and (out['y'] != S.points(n, nc, 3000 * nc + n)).any()
            cases[S.gradient_key(n, nc)] = entry(S.gradient_key(n, nc), out)
    path = os.path.join(HERE, 'ref_scan.json')
    with open(path, 'w') as f:
        f.write('{"cases": {\n%s\n}}\n' % ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(cases[k], sort_keys=True)) for k in sorted(cases)))
    print('wrote ref_scan.json', os.path.getsize(path), 'bytes;', len(cases), 'cases')


if __name__ == '__main__':
    main()
