"""CPU test of the slot arithmetic of the LDS Verlet lists (neuralmelting_amd/csrc/nm_math.h: list_slot, the expression the rebuild has always
used and the pair loop's reader mirrors, and list_slot_shifted, which the rebuild's append loop evaluates on the rank it carries pre-shifted):
the header is plain C++, compiled here for the host.  scripts/nm_list_slot_check.cpp walks every rank below the row capacity from every
starting rank, for every (threads per row, entries per word, rows, capacity) that a row of nm_rows.hip's table with LDS lists uses, and for
shapes none uses; list_slot compared with itself (the parent's expression on both sides) is the same walk and passes by construction."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table_shapes():
    """(log2 TPA, log2 PW, NLIST, MAXNB) of every Cfg typedef of nm_rows.hip whose list lives in LDS"""
    shapes = set()
    for line in open(os.path.join(ROOT, 'neuralmelting_amd', 'csrc', 'nm_rows.hip')):
        m = re.match(r'\s*typedef Cfg<([^>]*)> (\w+);', line)
        if not m:
            continue
        a = [t.strip() for t in m.group(1).split(',')]
        tpa, nmax, maxnb, idx, list_lds = int(a[1]), int(a[2]), int(a[3]), a[4], a[5] == 'true'
        if not list_lds:
            continue
        nlist = int(a[8]) if len(a) > 8 else nmax
        shapes.add((tpa.bit_length() - 1, 3 if idx == 'unsigned char' else 2, nlist, maxnb))
    return sorted(shapes)


def test_table_has_the_shapes_the_check_is_about():
    shapes = _table_shapes()
    assert {s[0] for s in shapes} >= {1, 2, 3, 4}              # 2 to 16 threads per row
    assert {s[1] for s in shapes} == {2, 3}                    # 16-bit and byte lists
    assert (3, 3, 64, 192) in shapes                           # the benchmark's row (256 atoms, 4 workgroups per replica)


def test_shifted_rank_gives_the_same_slot(tmp_path):
    exe = str(tmp_path / 'nm_list_slot_check')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'neuralmelting_amd', 'csrc'), '-o', exe,
                           os.path.join(ROOT, 'scripts', 'nm_list_slot_check.cpp')])
    shapes = _table_shapes() + [(0, 3, 256, 64), (0, 2, 8, 16), (4, 2, 5, 128), (2, 3, 1, 32)]   # one thread per row, odd row counts, one row
    r = subprocess.run([exe], input=''.join('%d %d %d %d\n' % s for s in shapes), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.split('\n') if l]
    assert len(lines) == len(shapes) and all(re.fullmatch(r'ok [1-9]\d*', l) for l in lines), r.stdout
