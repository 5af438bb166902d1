#!/usr/bin/env python3
"""tools/pass_static.py -- the pass kernels of two builds of fft.hip / domain.hip compared statically, kernel by kernel; one JSON line
per kernel (profiles/r20_pass_static.jsonl).  Needs no GPU.

  hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S fft.hip -o A/fft.s        (and domain.hip; the same for build B)
  python tools/pass_static.py A/fft.s B/fft.s; python tools/pass_static.py A/domain.s B/domain.s

Per side: the VGPR and SGPR counts, scratch and static LDS bytes of the kernel's metadata, and the counts of 64-bit multiply-adds,
LDS, global and barrier instructions, of all VALU and SALU instructions and of all instructions.  counts_equal: the first eight agree;
identical: the two instruction streams are the same text once the numbers of the local labels are dropped."""
import json
import re
import sys


def kernels(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:', txt, re.S | re.M):
        ins = [l.split(';')[0].strip() for l in m.group(2).split('\n')]
        out[m.group(1)] = {'body': [re.sub(r'\.LBB\d+_', '.LBB_', l) for l in ins if l and not l.startswith('.') and not l.endswith(':')]}
    for m in re.finditer(r'- \.agpr_count:.*?\.wavefront_size', txt, re.S):
        name = re.search(r'\.name:\s+(\S+)', m.group(0)).group(1)
        for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size'):
            if name in out:
                out[name][k] = int(re.search(r'\.%s:\s+(\d+)' % k, m.group(0)).group(1))
    return out


def short(name):
    m = re.search(r'(fft_pass_kernel|dom_pass_kernel)ILi(\d)(?:ELi(\d))?', name)
    return '%s<%s%s>' % (m.group(1), m.group(2), ',' + m.group(3) if m.group(3) else '') if m else None


def stats(k):
    n = lambda p: sum(1 for i in k['body'] if re.match(p, i))
    return dict(vgpr=k['vgpr_count'], sgpr=k['sgpr_count'], scratch=k['private_segment_fixed_size'], lds_static=k['group_segment_fixed_size'],
                mad64=n(r'v_mad_u64_u32'), ds=n(r'ds_'), glob=n(r'global_'), barrier=n(r's_barrier'), valu=n(r'v_'),
                salu=n(r's_(?!barrier|waitcnt|nop|endpgm)'), total=len(k['body']))


A, B = ({short(n): k for n, k in kernels(p).items() if short(n)} for p in sys.argv[1:3])
assert A and sorted(A) == sorted(B), (sorted(A), sorted(B))
for name in sorted(A):
    a, b = stats(A[name]), stats(B[name])
    print(json.dumps(dict(kernel=name, parent=a, branch=b, identical=A[name]['body'] == B[name]['body'],
                          counts_equal=all(a[k] == b[k] for k in ('vgpr', 'sgpr', 'scratch', 'lds_static', 'mad64', 'ds', 'glob', 'barrier')))))
