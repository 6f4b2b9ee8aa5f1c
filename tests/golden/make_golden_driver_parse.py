"""Golden fixture for the driver's files as the reference's consumer reads them: runs the driver with the oracle stand-in as its
engine (the run of tests/test_driver.py::test_driver_formats_with_oracle_engine) in a scratch directory, then the REFERENCE's own
scripts/lammps_parse.py, unmodified, as a child process on the files the driver left, and stores the two consolidated files, the
grid, and every array the script wrote (20 .npy files) in ref_driver_parse.npz.  That test replays it through
neuralmelting_amd.parse.

    NM_REFERENCE=<checkout of the reference> python tests/golden/make_golden_driver_parse.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
from helpers import OracleEngine  # noqa: E402
from make_golden_parse import NAMES  # noqa: E402
from neuralmelting_amd import remcmc  # noqa: E402
from oracle import oracle as O  # noqa: E402

ARGV = '-bm -n t1 -e LJ -ss 4 -pn 2 -tn 2 -sn 3 -sm 4 -sc 1 -rd 2'.split()


def main():
    ref = os.path.join(os.environ['NM_REFERENCE'], 'scripts', 'lammps_parse.py')
    O.build()
    O.lib()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        run = remcmc.Run(ARGV, cwd=d)
        run.make_engine = lambda: OracleEngine(O, run)
        run.main()
        pre = run.PREF
        out['P'], out['T'] = np.load(pre + '.virial.trgt.npy'), np.load(pre + '.temp.trgt.npy')
        out['thrm_txt'] = np.frombuffer(open(pre + '.thrm', 'rb').read(), dtype=np.uint8)
        out['traj_txt'] = np.frombuffer(open(pre + '.traj', 'rb').read(), dtype=np.uint8)
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
        subprocess.run([sys.executable, ref, '-n', 't1', '-e', 'LJ'], cwd=d, check=True, env=env)
        for n in NAMES:
            out['ref_' + n] = np.load(pre + '.%s.npy' % n)
    np.savez_compressed(os.path.join(HERE, 'ref_driver_parse.npz'), **out)
    print({k: (v.shape, str(v.dtype)) for k, v in out.items() if k.startswith('ref_')})


if __name__ == '__main__':
    main()
