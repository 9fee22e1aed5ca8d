"""Is the device code of two versions of csrc/ the same, kernel by kernel (no GPU needed)?

    git worktree add /tmp/parent HEAD~1
    python tools/device_code_diff.py /tmp/parent/safe_exploration_amd/csrc safe_exploration_amd/csrc [-j JOBS]

Compiles every .hip of both directories to gfx950 assembly with the library's device flags (each directory must sit in
its tree: the sources include ../../include/sx_amd.h), splits the assembly into functions and compares, per kernel symbol,
the instruction text, the .amdhsa_kernel descriptor block and the kernel's entry in the amdhsa.kernels metadata.  Label
numbers, comments and section directives are ignored (they count functions per translation unit), so a kernel may move
from one translation unit to another and still compare equal.  Prints the kernels only one side has, the kernels a side
compiles more than once (two translation units would each register a copy: the LDS grants and device symbols are keyed on
one), and the kernels that differ, with the first differing line; exits 1 if there is any of them.  A kernel whose
symbol only one side has is then looked for on the other side by content (its own symbol replaced by a placeholder in
all three parts): a template that gained a parameter renames every instantiation, and such a kernel is reported as
`renamed` and counts as identical, not as a finding.  --added REGEX names the kernels a change adds on purpose: a symbol
only the new side has that matches is printed as `added` and is no finding either.  DESIGN.md section 3.5 describes the method.  SX_EXTRA_FLAGS is
passed on as csrc/build.sh does.
"""
import argparse
import concurrent.futures
import glob
import os
import re
import shlex
import subprocess
import sys
import tempfile

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-mllvm', '-amdgpu-mfma-vgpr-form=1', '--cuda-device-only', '-S']

_LABEL = re.compile(r'\.L([A-Za-z_]+?)\d+(_\d+)?\b')      # .LBB12_3 -> .LBB_3, .Lfunc_end12 -> .Lfunc_end


def _clean(lines):
    """Instruction text: no comments, no section directives, labels without the function's number."""
    out = []
    for line in lines:
        line = line.split(';', 1)[0].rstrip()
        s = line.strip()
        if not s or s.startswith(('.section', '.text', '.p2align', '.set ')):
            continue
        out.append(_LABEL.sub(lambda m: '.L' + m.group(1) + (m.group(2) or ''), s))
    return out


def kernels_of(asm):
    """{kernel symbol: (instructions, descriptor, metadata)} of one translation unit's assembly; a list per symbol."""
    lines = asm.split('\n')
    found = {}
    i = 0
    while i < len(lines):
        m = re.match(r'\s*\.type\s+(\S+),@function', lines[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        end = next(j for j in range(i, len(lines)) if re.match(r'\s*\.size\s+' + re.escape(name) + ',', lines[j]))
        body = lines[i + 1:end]
        i = end + 1
        starts = [j for j, l in enumerate(body) if l.strip().startswith('.amdhsa_kernel ')]
        if not starts:
            continue                                         # a device function, not a kernel
        stop = next(j for j in range(starts[0], len(body)) if body[j].strip() == '.end_amdhsa_kernel')
        found[name] = [_clean(body[:starts[0]] + body[stop + 1:]), _clean(body[starts[0]:stop + 1])]
    meta = asm[asm.index('amdhsa.kernels:'):] if 'amdhsa.kernels:' in asm else ''
    meta = re.split(r'\namdhsa\.[a-z]+:', meta[len('amdhsa.kernels:'):])[0]
    for entry in re.split(r'\n  - ', meta)[1:]:
        name = re.search(r'\.symbol:\s+(\S+)\.kd', entry).group(1)
        found[name].append([l.rstrip() for l in entry.split('\n') if l.strip() and not l.startswith('...')])
    return found


def compile_dir(csrc, jobs):
    """{kernel symbol: [(source file, parts), ...]} over every .hip of `csrc`."""
    csrc = os.path.abspath(csrc)
    srcs = sorted(glob.glob(os.path.join(csrc, '*.hip')))
    if not srcs:
        sys.exit(f'no .hip files in {csrc}')
    extra = shlex.split(os.environ.get('SX_EXTRA_FLAGS', ''))
    with tempfile.TemporaryDirectory() as tmp:
        def one(src):
            out = os.path.join(tmp, os.path.basename(src) + '.s')
            subprocess.check_call([HIPCC] + FLAGS + extra + [src, '-o', out], cwd=csrc, stderr=subprocess.DEVNULL)
            return open(out).read()
        with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
            texts = list(pool.map(one, srcs))
    table = {}
    for src, text in zip(srcs, texts):
        for name, parts in kernels_of(text).items():
            table.setdefault(name, []).append((os.path.basename(src), parts))
    return table


def first_difference(a, b):
    for n, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f'line {n}: {x!r} | {y!r}'
    return f'{len(a)} lines | {len(b)} lines'


def _anonymous(name, parts):
    """The three parts of a kernel with its own symbol replaced by a placeholder, hashable."""
    return tuple(tuple(line.replace(name, '<kernel>') for line in part) for part in parts)


def renamed(old, new):
    """{old symbol: new symbol} of the kernels whose symbol only one side has and whose parts are equal but for the symbol."""
    by_content = {}
    for name in sorted(set(new) - set(old)):
        by_content.setdefault(_anonymous(name, new[name][0][1]), []).append(name)
    pairs = {}
    for name in sorted(set(old) - set(new)):
        twins = by_content.get(_anonymous(name, old[name][0][1]))
        if twins:
            pairs[name] = twins.pop(0)
    return pairs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('old_csrc')
    ap.add_argument('new_csrc')
    ap.add_argument('-j', '--jobs', type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument('--added', metavar='REGEX', help='kernels only the new side has whose symbol matches are the change\'s '
                    'own: printed as `added`, not counted as findings')
    args = ap.parse_args()
    old, new = compile_dir(args.old_csrc, args.jobs), compile_dir(args.new_csrc, args.jobs)
    bad = 0
    pairs = renamed(old, new)
    for a, b in sorted(pairs.items()):
        print(f'renamed: {a} ({old[a][0][0]}) -> {b} ({new[b][0][0]})')
    moved = set(pairs) | set(pairs.values())
    added = 0
    for side, here, there in (('old', old, new), ('new', new, old)):
        for name in sorted(set(here) - set(there) - moved):
            if side == 'new' and args.added and re.search(args.added, name):
                print(f'added: {name} ({here[name][0][0]})')
                added += 1
                continue
            print(f'only in {side}: {name} ({here[name][0][0]})')
            bad += 1
        for name in sorted(here):
            if len(here[name]) > 1:
                print(f'{len(here[name])} copies in {side}: {name} ({", ".join(f for f, _ in here[name])})')
                bad += 1
    same = 0
    for name in sorted(set(old) & set(new)):
        (fo, po), (fn, pn) = old[name][0], new[name][0]
        diffs = [f'{what}: {first_difference(x, y)}'
                 for what, x, y in zip(('instructions', 'descriptor', 'metadata'), po, pn) if x != y]
        if diffs:
            print(f'differs: {name} ({fo} -> {fn})')
            for d in diffs:
                print('    ' + d)
            bad += 1
        else:
            same += 1
    print(f'{len(old)} kernels in old, {len(new)} in new, {same} identical, {len(pairs)} renamed and identical, '
          f'{added} added, {bad} findings')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
