"""Golden fixture for the VAE stage: runs the cases of tests/vae_cases.py through the library as it is built in this tree (or the one
that NM_HIP_LIB names), on the GPU, and stores the shape, the dtype and the SHA-256 of every output's bytes in ref_vae.json, small
outputs in full as well, so that a mismatch can be read.  The stage is deterministic, so the fixture pins its bytes: every case
runs twice first, and nothing is written if any digest differs between the two runs (that would be a finding about the library).

It was run once, on an MI355X, on the library of the commit before the network of csrc/nm_vae_api.hip was put into one table of
layers, and is not run again to make a failing test pass: a refactor that changes a byte is wrong.

    python tests/golden/make_golden_vae.py"""
import json
import os
import sys

import numpy as np

os.environ['PYTHONDONTWRITEBYTECODE'] = '1'
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
import vae_cases as V  # noqa: E402


def run(key, case):
    out = case()
    for name, a in out.items():
        assert np.isfinite(a).all() and (a != V.SENTINEL).all(), (key, name)
    if 'grad' in out:                                               # no parameter tensor without a gradient, none left where it was
        side, latent = (int(w.lstrip('sld')) for w in key.split('_')[1:3])
        off = np.zeros(V.B.NM_VAE_NTENSORS + 1, dtype=np.int64)
        assert V.B.load().nm_vae_layout(side, latent, off) == V.B.NM_OK
        theta = V.params(side, latent)
        for t in range(V.B.NM_VAE_NTENSORS):
            assert out['grad'][off[t]:off[t + 1]].any() and (out['params'][off[t]:off[t + 1]] != theta[off[t]:off[t + 1]]).any(), (key, t)
    return {'outputs': {name: V.digest(a) for name, a in out.items()}}


def main():
    first = {key: run(key, case) for key, case in V.every_case()}
    again = {key: run(key, case) for key, case in V.every_case()}
    differ = [(key, name) for key in first for name in first[key]['outputs'] if first[key]['outputs'][name] != again[key]['outputs'][name]]
    if differ:
        print('NOT written: these outputs differ between two runs of the same case:', differ)
        return 1
    path = os.path.join(HERE, 'ref_vae.json')
    with open(path, 'w') as f:
        f.write('{"cases": {\n%s\n}}\n' % ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(first[k], sort_keys=True)) for k in sorted(first)))
    print('wrote ref_vae.json', os.path.getsize(path), 'bytes;', len(first), 'cases of', V.B.LIB_PATH)
    return 0


if __name__ == '__main__':
    sys.exit(main())
