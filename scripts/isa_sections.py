#!/usr/bin/env python3
"""Per-section instruction counts of one row's production kernels (developer tool: it counts, it asserts nothing).

The production kernels of a row of nm_rows.hip's table (nm_cycles_kernel<Cfg, false, true> and nm_block_kernel<Cfg, true>) are compiled
ALONE, each from an explicit instantiation in a few lines of HIP that include nm_kernels.h, with -gline-tables-only, and every instruction of
the assembly is attributed through its .loc line to the source function that line lies in (the innermost inlined function: .loc names the
line an instruction came from, not the caller's; code without a line, which is most spill code, goes with the line before it).  Two tables
per kernel: the whole kernel with the functions it calls (gaussian_fill, velocity_create), and the stretch that is one force-only step of a
trajectory (the body of nm_block_body's loop over them, the rarely taken rebuild included).  --check-lines compiles once more without line
tables and compares the instruction streams: the kernels come out the same, the two called functions save exec in their prologues where
there is frame information to describe it (four v_writelane in all, profiles/r23_scalar_diet.txt).

The compiler's output for a kernel depends on what else its translation unit holds (profiles/r22_split_sampler.txt), so these tables are the
working proxy while code is being changed; the figures of record come from `make resources` and `make asm` of the whole nm_rows.hip.

    scripts/isa_sections.py CfgSmallQ4                      # fused and block kernel of the row
    scripts/isa_sections.py CfgSmallSCQ4 --kernel fused --check-lines
    scripts/isa_sections.py CfgSmallQ4 --src other/checkout/neuralmelting_amd/csrc --keep /tmp/q4
    scripts/isa_sections.py CfgSmallQ4 --keep /tmp/q4 --reuse   # count the kept assembly again
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {
    'fused': 'template __global__ void nm_cycles_kernel<%s, false, true>(const KParams);',
    'block': 'template __global__ void nm_block_kernel<%s, true>(const KParams);',
}
# source function -> section of the report (functions not named here report under their own name if they hold >= MIN_OWN instructions,
# else under `other`)
SECTION_OF = {
    'rebuild': 'rebuild', 'rebuild_rows_hbm': 'rebuild', 'test16': 'rebuild', 'block_scan': 'rebuild', 'nbr_at': 'rebuild', 'lrow': 'rebuild',
    'pair_loop': 'pair_loop (outside trips)', 'pair_loop_sc': 'pair_loop (outside trips)', 'group_sum': 'pair_loop (outside trips)',
    'dpp_shl': 'pair_loop (outside trips)', 'dpp_mov': 'pair_loop (outside trips)', 'prio_begin': 'pair_loop (outside trips)',
    'prio_swap': 'pair_loop (outside trips)', 'prio_end': 'pair_loop (outside trips)', 'young': 'pair_loop (outside trips)',
    'put_granule': 'put_granule', 'get_granules': 'get_granules', 'magic_at': 'magic', 'magic': 'magic', 'my_magic': 'magic',
    'pair_pre': 'neighbour trips', 'pair_vec': 'neighbour trips', 'pair_vec_half': 'neighbour trips', 'recip': 'neighbour trips',
    'sc_rho_vec': 'neighbour trips', 'sc_force_vec': 'neighbour trips', 'sc_rep': 'neighbour trips', 'sc_at': 'neighbour trips',
    'eval_force': 'eval_force', 'eval': 'eval', 'box_consts': 'box_consts', 'check_begin': 'list check', 'check_atom': 'list check',
    'advance_and_share': 'advance_and_share',
    'block_sum': 'block reductions', 'block_any': 'block reductions', 'block_any2': 'block reductions', 'block_any3': 'block reductions',
    'wave_sum': 'block reductions', 'uniform': 'block reductions',
    'exchange_sums': 'exchange_sums', 'finish_sums': 'exchange_sums', 'take_sums': 'exchange_sums',
    'velocity_create': 'velocity_create', 'hmc_velocities': 'velocity_create', 'gaussian_fill': 'gaussian_fill',
    'nm_block_body': 'move loop (nm_block_body)', 'metropolis': 'move loop (nm_block_body)', 'draw_scalar': 'move loop (nm_block_body)',
    'draw_tag': 'move loop (nm_block_body)', 'q6': 'move loop (nm_block_body)',
    'save': 'save/restore/wrap', 'restore': 'save/restore/wrap', 'wrap': 'save/restore/wrap', 'wrap1': 'save/restore/wrap',
    'load': 'load/store', 'store': 'load/store', 'philox4x32_10': 'philox', 'u01': 'philox',
    'nm_cycles_kernel': 'cycle tail (nm_cycles_kernel)', 'residency_census': 'census',
}
MIN_OWN = 40
COLUMNS = ('insts', 'lane', 'scratch', 's_nop', 's_waitcnt', 'div_f64')


def function_ranges(path):
    """[(first line, last line, name)] of every function defined in a header, by the braces that follow a __device__/__global__ declarator;
    plus, inside pair_loop and pair_loop_sc, the loops over a row's list words (`for (int k0 ...`) as ('neighbour trips')"""
    text = open(path).read()
    # comments and strings out of the way of the brace count (lengths kept, so offsets stay line-true)
    def blank(m):
        return re.sub(r'[^\n]', ' ', m.group(0))
    clean = re.sub(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'', blank, text, flags=re.S)
    line_of = [0] * (len(clean) + 1)
    n = 1
    for k, ch in enumerate(clean):
        line_of[k] = n
        if ch == '\n':
            n += 1
    line_of[len(clean)] = n

    def body_end(open_at):
        depth = 0
        for k in range(open_at, len(clean)):
            if clean[k] == '{':
                depth += 1
            elif clean[k] == '}':
                depth -= 1
                if depth == 0:
                    return k
        return len(clean) - 1

    out = []
    for m in re.finditer(r'(__device__|__global__)[^;{}()]*?(?:Replica<C, PLAIN>::)?(\w+)\s*\(', clean):
        name = m.group(2)
        if name in ('__launch_bounds__', '__attribute__', 'noinline'):
            # the declarator goes on behind the attribute: take the next identifier in front of a parenthesis
            m2 = re.compile(r'\)\s*\)?\s*[\w:<>,\s\*&]*?(\w+)\s*\(').search(clean, m.end())
            if not m2:
                continue
            name, start = m2.group(1), m2.end()
        else:
            start = m.end()
        # the parameter list, then either ';' (a declaration) or the body
        depth, k = 1, start
        while k < len(clean) and depth:
            depth += {'(': 1, ')': -1}.get(clean[k], 0)
            k += 1
        m3 = re.compile(r'\s*(const)?\s*(:[^{;]*)?([{;])', re.S).match(clean, k)
        if not m3 or m3.group(3) == ';':
            continue
        open_at = m3.end() - 1
        end = body_end(open_at)
        out.append((line_of[m.start()], line_of[end], name))
        if name in ('pair_loop', 'pair_loop_sc'):
            for t in re.finditer(r'for \(int k0\b[^{]*\{', clean[open_at:end]):
                o = open_at + t.end() - 1
                out.append((line_of[open_at + t.start()], line_of[body_end(o)], 'pair_vec'))  # reports as neighbour trips
    return out


def section_lookup(srcdir):
    tables = {}
    for h in ('nm_kernels.h', 'nm_device.h', 'nm_math.h'):
        p = os.path.join(srcdir, h)
        if os.path.exists(p):
            tables[h] = function_ranges(p)

    def lookup(fname, line):
        best = None
        for a, b, name in tables.get(os.path.basename(fname), ()):
            if a <= line <= b and (best is None or b - a < best[0]):
                best = (b - a, name)  # the innermost range that holds the line
        return best[1] if best else os.path.basename(fname)
    return lookup


def cfg_typedef(srcdir, cfg):
    for line in open(os.path.join(srcdir, 'nm_rows.hip')):
        m = re.match(r'\s*typedef (Cfg<.*>) %s;' % re.escape(cfg), line)
        if m:
            return m.group(1)
    sys.exit('no typedef of %s in nm_rows.hip' % cfg)


def compile_one(srcdir, cfg, kind, outdir, lines=True, flags=()):
    stem = os.path.join(outdir, '%s_%s%s' % (cfg, kind, '' if lines else '_nolines'))
    with open(stem + '.hip', 'w') as f:
        f.write('#include "%s/../../include/nm.h"\n#include "%s/nm_rows.h"\n#include "%s/nm_kernels.h"\n' % (srcdir, srcdir, srcdir))
        f.write('namespace nm { typedef %s %s;\n%s }\n' % (cfg_typedef(srcdir, cfg), cfg, KERNELS[kind] % cfg))
    cmd = [os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-O3', '-std=c++17', '--offload-arch=' + os.environ.get('ARCH', 'gfx950'),
           '--cuda-device-only', '-S', '-Rpass-analysis=kernel-resource-usage', '-o', stem + '.s', stem + '.hip']
    if lines:
        cmd.insert(1, '-gline-tables-only')
    cmd[1:1] = flags
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        sys.exit(r.stdout)
    return ' '.join(cmd), stem + '.s', r.stdout


INST = re.compile(r'^\t([a-z_][a-z0-9_]*)\b')
FUNC = re.compile(r'^\t\.type\t(\S+),@function')


def wanted_functions(path, kind):
    """the requested kernel and the device functions that are not inlined into it (gaussian_fill, velocity_create); the small kernels that
    nm_kernels.h defines beside them (order, record, adapt, exchange) are in the translation unit but not in the report"""
    text = open(path).read()
    kernels = set(re.findall(r'^\t\.amdhsa_kernel (\S+)', text, flags=re.M))
    target = {'fused': 'nm_cycles_kernel', 'block': 'nm_block_kernel'}[kind]
    return lambda fn: fn is not None and (fn not in kernels or target in fn)


def instructions(path, kind):
    """(function symbol, (file, line), mnemonic, text) of every instruction of the wanted functions.  An instruction with line 0 (code the
    compiler made up: most spill code) goes with the last line named before it"""
    want = wanted_functions(path, kind)
    files, fn, cur = {}, None, ('?', 0)
    for line in open(path):
        if line.startswith('\t.file\t'):
            m = re.match(r'\t\.file\t(\d+) "([^"]*)"(?: "([^"]*)")?', line)
            if m:
                files[int(m.group(1))] = m.group(3) or m.group(2)
            continue
        m = FUNC.match(line)
        if m:
            fn, cur = m.group(1), ('?', 0)
            continue
        if line.startswith('\t.section') and '.text' not in line or line.startswith('\t.amdhsa_kernel'):
            fn = None
            continue
        if line.startswith('\t.loc\t'):
            t = line.split()
            if int(t[2]) != 0:
                cur = (files.get(int(t[1]), '?'), int(t[2]))
            continue
        m = INST.match(line)
        if m and want(fn):
            yield fn, cur, m.group(1), line.split(';')[0].strip()


def stream(path, kind):
    return [t for _, _, _, t in instructions(path, kind)]


def step_lines(srcdir):
    """the source lines of one force-only trajectory step: the body of nm_block_body's loop over the nstps - 1 force-only evaluations"""
    lines = open(os.path.join(srcdir, 'nm_kernels.h')).read().split('\n')
    for k, l in enumerate(lines):
        if re.search(r'for \(.*\bs < nfo;', l):
            depth = 0
            for e in range(k, len(lines)):
                depth += lines[e].count('{') - lines[e].count('}')
                if depth == 0 and e > k:
                    return k + 1, e + 1
    return None


def count(path, kind, lookup, region=None):
    """region (first, last source line of nm_kernels.h): only the stretch of the kernel from the first to the last instruction that comes
    from those lines — with everything inlined into it — is counted"""
    sect, total, per_fn = {}, dict.fromkeys(COLUMNS, 0), {}
    insts = list(instructions(path, kind))
    if region:
        hit = [k for k, (fn, cur, _, _) in enumerate(insts)
               if os.path.basename(cur[0]) == 'nm_kernels.h' and region[0] <= cur[1] <= region[1] and 'kernel' in fn]
        insts = insts[hit[0]:hit[-1] + 1] if hit else []
    for _, cur, op, _ in insts:
        c = per_fn.setdefault(lookup(*cur), dict.fromkeys(COLUMNS, 0))
        c['insts'] += 1
        c['lane'] += op.startswith('v_readlane') or op.startswith('v_writelane')
        c['scratch'] += op.startswith('scratch_')
        c['s_nop'] += op == 's_nop'
        c['s_waitcnt'] += op == 's_waitcnt'
        c['div_f64'] += op == 'v_div_fmas_f64'
    for fn, c in per_fn.items():
        s = SECTION_OF.get(fn) or (fn if c['insts'] >= MIN_OWN else 'other')
        d = sect.setdefault(s, dict.fromkeys(COLUMNS, 0))
        for k in COLUMNS:
            d[k] += c[k]
            total[k] += c[k]
    return sect, total


def resources(remarks, kind):
    """the compiler's register and spill remarks of the wanted functions, one line each"""
    target = {'fused': 'nm_cycles_kernel', 'block': 'nm_block_kernel'}[kind]
    out, name = [], None
    for r in remarks.splitlines():
        m = re.search(r'remark: .*?Function Name: (\S+)', r)
        if m:
            name = m.group(1)
            keep = target in name or not re.search(r'nm_\w+_kernel', name)
            if keep:
                out.append([re.sub(r'INS_3Cfg.*', '<...>', name)])
            continue
        m = re.search(r'remark: .*?\s((?:SGPRs|VGPRs|AGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\])): (\d+)', r)
        if m and name and keep and m.group(1) in ('SGPRs', 'VGPRs', 'SGPRs Spill', 'VGPRs Spill', 'ScratchSize [bytes/lane]'):
            out[-1].append('%s %s' % (m.group(1).replace(' [bytes/lane]', ''), m.group(2)))
    return ['%s: %s' % (o[0], ', '.join(o[1:])) for o in out]


def report(title, cmd, remarks, sect, total):
    print('== %s' % title)
    print('   %s' % cmd)
    for r in remarks:
        print('   ' + r)
    print('   %-32s %7s %9s %8s %6s %9s %8s' % ('section', 'insts', 'rd/wrlane', 'scratch_', 's_nop', 's_waitcnt', 'div f64'))
    for s in sorted(sect, key=lambda s: -sect[s]['insts']):
        print('   %-32s %7d %9d %8d %6d %9d %8d' % ((s,) + tuple(sect[s][k] for k in COLUMNS)))
    print('   %-32s %7d %9d %8d %6d %9d %8d' % (('total',) + tuple(total[k] for k in COLUMNS)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('cfg', help='a Cfg typedef of nm_rows.hip with a production form, e.g. CfgSmallQ4')
    ap.add_argument('--kernel', choices=('fused', 'block', 'both'), default='both')
    ap.add_argument('--src', default=os.path.join(ROOT, 'neuralmelting_amd', 'csrc'), help='the csrc directory to compile (another checkout: a before/after pair)')
    ap.add_argument('--keep', help='directory that keeps the .hip and .s files')
    ap.add_argument('--flag', action='append', default=[], help='one more compiler flag, e.g. --flag=-DNM_EXPERIMENT (repeatable)')
    ap.add_argument('--reuse', action='store_true', help='count the assembly that an earlier run left in --keep; compile nothing')
    ap.add_argument('--check-lines', action='store_true', help='also compile without line tables and compare the instruction streams')
    a = ap.parse_args()
    srcdir = os.path.abspath(a.src)
    kinds = ('fused', 'block') if a.kernel == 'both' else (a.kernel,)
    outdir = a.keep or tempfile.mkdtemp(prefix='isa_sections_')
    os.makedirs(outdir, exist_ok=True)
    lookup = section_lookup(srcdir)
    jobs = [(k, True) for k in kinds] + ([(k, False) for k in kinds] if a.check_lines else [])
    if a.reuse:
        res = {j: ('(kept assembly)', os.path.join(outdir, '%s_%s%s.s' % (a.cfg, j[0], '' if j[1] else '_nolines')), '') for j in jobs}
    else:
        with concurrent.futures.ThreadPoolExecutor(len(jobs)) as ex:
            res = dict(zip(jobs, ex.map(lambda j: compile_one(srcdir, a.cfg, j[0], outdir, j[1], a.flag), jobs)))
    for k in kinds:
        cmd, s, remarks = res[(k, True)]
        sect, total = count(s, k, lookup)
        report('%s, %s kernel' % (a.cfg, k), cmd, resources(remarks, k), sect, total)
        if step_lines(srcdir):
            sect, total = count(s, k, lookup, step_lines(srcdir))
            report('%s, %s kernel: one force-only trajectory step (nm_kernels.h:%d-%d and what is inlined there; the rebuild runs in few steps)'
                   % ((a.cfg, k) + step_lines(srcdir)), '(same assembly)', [], sect, total)
        if a.check_lines:
            with_, without = stream(s, k), stream(res[(k, False)][1], k)
            d = [l for l in difflib.unified_diff(without, with_, lineterm='', n=0) if l[:1] in '+-' and l[:3] not in ('+++', '---')]
            print('   without -gline-tables-only: %d instructions against %d; %s' % (len(without), len(with_), 'identical stream' if not d else '%d lines differ:' % len(d)))
            for l in d[:20]:
                print('      ' + l)


if __name__ == '__main__':
    main()
