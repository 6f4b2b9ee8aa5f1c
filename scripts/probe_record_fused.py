"""Recorded cycles inside the fused launch, measured on the driver: the C2 run (-bm -e LJ -ss 4 -pn 8 -tn 8 -sm 128 -sn 256 -rd 100000) in ONE process
on one GPU, three arms alternated so that the box's drift falls on all of them alike:
  (a) -sc 0              every cycle recorded: nm_run_cycles_recorded, one fused launch per stretch of recorded cycles;
  (b) -sc 0, NM_FUSED_CYCLES=0   the same calls on the loop of single launches (a record copy behind every block);
  (c) -sc 100000         outputs off: nm_run_cycles;
  (d) -sc 0, files not written   (a) with write_outputs a no-op: the records are taken, copied and fetched, nothing is formatted — (a) against (d) is
                                 the writer thread's share, (d) against (c) the records' own (kernel stores, the ring's D2H, the fetches).
MC sweeps/s from remcmc.Run.loop_seconds (the main loop, files written and joined), without -v (verbose synchronises every exchange).
    python scripts/probe_record_fused.py [--repeats 3] [--out FILE]"""
import argparse
import os
import shutil
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from neuralmelting_amd import remcmc  # noqa: E402

BASE = '-bm -e LJ -ss 4 -pn 8 -tn 8 -sm 128 -sn 256 -rd 100000 -n probe'.split()
ARMS = (('a recorded, fused', ['-sc', '0'], None), ('b recorded, single launches', ['-sc', '0'], '0'), ('c outputs off', ['-sc', '100000'], None),
        ('d recorded, fused, no files', ['-sc', '0'], 'nowrite'))


def one(argv, fused_env):
    d = tempfile.mkdtemp(prefix='nm_probe_')
    old = os.environ.pop('NM_FUSED_CYCLES', None)
    try:
        if fused_env not in (None, 'nowrite'):
            os.environ['NM_FUSED_CYCLES'] = fused_env
        run = remcmc.Run(argv, cwd=d)
        if fused_env == 'nowrite':
            run.write_outputs = lambda rows, x, box: None
            run.consolidate_outputs = lambda: None     # (behind the timed loop; there are no frames to gather)
        run.main()
        return run.nloc * run.MOD * run.NSMPL / run.loop_seconds
    finally:
        os.environ.pop('NM_FUSED_CYCLES', None)
        if old is not None:
            os.environ['NM_FUSED_CYCLES'] = old
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = ['# %s' % ' '.join(BASE)]
    one(BASE + ['-sc', '0', '-sn', '8'], None)      # warm-up: code objects loaded, files system warm
    res = {name: [] for name, _, _ in ARMS}
    for r in range(a.repeats):
        for name, extra, env in ARMS:
            s = one(BASE + extra, env)
            res[name].append(s)
            lines.append('repeat %d  %-30s %10.0f sweeps/s' % (r, name, s))
            print(lines[-1], flush=True)
    for name, _, _ in ARMS:
        v = np.array(res[name])
        lines.append('%-30s median %10.0f  min %10.0f  max %10.0f  (spread %.2f %%)' % (name, np.median(v), v.min(), v.max(),
                                                                                       100 * (v.max() - v.min()) / np.median(v)))
    ra = np.array(res[ARMS[0][0]]) / np.array(res[ARMS[2][0]])
    rb = np.array(res[ARMS[1][0]]) / np.array(res[ARMS[2][0]])
    lines.append('recorded fused / outputs off, per repeat: %s  median %.4f' % (' '.join('%.4f' % x for x in ra), np.median(ra)))
    lines.append('recorded single launches / outputs off, per repeat: %s  median %.4f' % (' '.join('%.4f' % x for x in rb), np.median(rb)))
    rd = np.array(res[ARMS[3][0]]) / np.array(res[ARMS[2][0]])
    lines.append('recorded fused, no files / outputs off, per repeat: %s  median %.4f' % (' '.join('%.4f' % x for x in rd), np.median(rd)))
    text = '\n'.join(lines) + '\n'
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
