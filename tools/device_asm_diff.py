"""Diff the gfx950 device assembly of two checkouts, symbol by symbol (no GPU needed).

    python tools/device_asm_diff.py OLD_CHECKOUT NEW_CHECKOUT [old=new ...]

Every entry of each checkout's build.SOURCES is compiled with that checkout's own FLAGS and EXTRA plus
`-fuse-cuid=none --offload-device-only -S` (reproducible, carries no path).  The output is split at symbol labels; local
labels (.LBB<function>_<block>, ...) lose their function number, which shifts when a neighbour is deleted.  Reported:
symbols on one side only, and symbols whose bodies differ after the `old=new` renames (plain substring substitutions on
the OLD text, e.g. for a template parameter list that got shorter) are applied.  Exit status 1 when a body differs or a
symbol exists only in NEW.
"""
import os
import re
import runpy
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LABEL = re.compile(r'^([A-Za-z_$][\w$.]*):')
LOCAL = re.compile(r'(\.L[A-Za-z_]+|\bBB)\d+')      # .LBB86_12, .Lfunc_end86, and BB86_12 in loop comments
PAD = re.compile(r'[ \t]+;')                           # the comment column moves with the label's width
# a symbol's own preamble is emitted before its label, i.e. at the tail of its predecessor: not part of either body
PREAMBLE = re.compile(r'^\s*\.(globl|weak|protected|hidden|p2align|type|section|text|data|bss)\b')


def device_asm(root, tmp):
    """{source: assembly text} of one checkout."""
    b = runpy.run_path(os.path.join(root, 'vqcpc_bach_amd', 'build.py'))
    jobs = []
    for src in b['SOURCES']:
        out = os.path.join(tmp, src + '.s')
        jobs.append((src, out, [b['_hipcc']()] + b['FLAGS'] + b['EXTRA'].get(src, []) +
                     ['-fuse-cuid=none', '--offload-device-only', '-S', os.path.join(b['CSRC'], src), '-o', out]))
    with ThreadPoolExecutor(max_workers=min(len(jobs), int(os.environ.get('MAX_JOBS', 16)))) as pool:
        list(pool.map(lambda j: subprocess.check_call(j[2]), jobs))
    return {src: open(out).read() for src, out, _ in jobs}


def symbols(asm, renames=()):
    """{'file:symbol': body} -- the text from each non-local label up to the next one (or the metadata note)."""
    syms = {}
    for src, text in asm.items():
        for old, new in renames:
            text = text.replace(old, new)
        name = None
        for line in text.split('\n'):
            if line.lstrip().startswith('.amdgpu_metadata'):
                break
            m = LABEL.match(line)
            if m:
                name = src + ':' + m.group(1)
                syms[name] = []
            elif name and not PREAMBLE.match(line):
                syms[name].append(PAD.sub(' ;', LOCAL.sub(r'\1', line)))
    return syms


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    renames = [tuple(a.split('=', 1)) for a in argv[3:]]
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new:
        old = symbols(device_asm(argv[1], t_old), renames)
        new = symbols(device_asm(argv[2], t_new))
    only_old = sorted(set(old) - set(new))
    only_new = sorted(set(new) - set(old))
    differ = sorted(s for s in set(old) & set(new) if old[s] != new[s])
    for title, names in (('only in OLD', only_old), ('only in NEW', only_new), ('body differs', differ)):
        print('%s: %d' % (title, len(names)))
        for s in names:
            print('    ' + s)
    print('symbols: %d old, %d new, %d common, %d identical' %
          (len(old), len(new), len(set(old) & set(new)), len(set(old) & set(new)) - len(differ)))
    return 1 if only_new or differ else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
