"""CPU test of the predicate that accepts a handed-over granule (neuralmelting_amd/csrc/nm_math.h: granule_state, used by nm_kernels.h
get_granules for one to four granules per poll): the header is plain C++, compiled here for the host.  With x = word0 ^ word1 ^ magic the
exact test is x == 0 (valid) or x == POISON (valid, the publisher's list overflowed); everything else is a torn or stale granule — in
particular every word that merely has no bit outside POISON, which a cheaper test would accept."""
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0x5555555555555554
INVALID, VALID, POISONED = 0, 1, 2


def _cases():
    bits = [1 << k for k in range(64)]
    cases = [(0, VALID), (POISON, POISONED)]
    cases += [(b, INVALID) for b in bits]                                   # every single-bit change of 0 ...
    cases += [(POISON ^ b, INVALID) for b in bits]                          # ... and of POISON (its set bits cleared one by one among them)
    cleared = [POISON & ~b for b in bits if POISON & b]
    assert len(cleared) == 31
    cases += [(w, INVALID) for w in cleared]
    rng = random.Random(20240624)
    for _ in range(4096):
        w = rng.getrandbits(64)
        cases.append((w, INVALID))
        cases.append((w & POISON, INVALID))                                 # no bit outside POISON: still torn
        cases.append((w | POISON, INVALID))
    # (a random word that happens to be one of the two valid ones would be expected as such: none is, with this seed)
    return [(w, VALID if w == 0 else POISONED if w == POISON else want) for w, want in cases]


def test_granule_state_is_the_exact_test(tmp_path):
    exe = str(tmp_path / 'nm_granule_check')
    subprocess.check_call(['g++', '-O2', '-I', os.path.join(ROOT, 'neuralmelting_amd', 'csrc'), '-o', exe,
                           os.path.join(ROOT, 'scripts', 'nm_granule_check.cpp')])
    cases = _cases()
    assert sum(want == VALID for _, want in cases) == 1 and sum(want == POISONED for _, want in cases) == 1
    r = subprocess.run([exe], input=''.join('%x\n' % w for w, _ in cases), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split('\n')
    assert lines[0] == 'poison %x' % POISON                                 # the kernels' constant is the one these cases are built on
    got = [int(l) for l in lines[1:] if l]
    assert len(got) == len(cases)
    wrong = [('%016x' % w, want, g) for (w, want), g in zip(cases, got) if g != want]
    assert not wrong, wrong[:10]
