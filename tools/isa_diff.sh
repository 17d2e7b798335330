#!/bin/bash
# Compare the gfx950 ISA of two objects kernel by kernel (instruction text only, addresses stripped):
#   tools/isa_diff.sh old.o new.o [kernel-name-fragment]
# Used to prove that a refactoring left a hot kernel's code untouched.
set -u
B=/opt/rocm/lib/llvm/bin
for tag in a b; do
  f=$1; [ $tag = b ] && f=$2
  $B/llvm-objcopy -O binary --only-section=.hip_fatbin $f /tmp/isa_$tag.fb
  $B/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=/tmp/isa_$tag.fb --output=/tmp/isa_$tag.co
  $B/llvm-objdump -d --no-show-raw-insn /tmp/isa_$tag.co | sed -E 's/^\s*([a-z_0-9]+.*)\/\/ [0-9A-F]+:.*$/\1/; s/\s+$//' > /tmp/isa_$tag.txt
done
python3 - "${3:-}" <<'PY'
import re, sys
frag = sys.argv[1]
def kernels(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', ln.strip())
        if m:
            cur = re.sub(r'8ZeroFilljj$', '8ZeroFill', m.group(1))
            # the generic wave kernels before they lost their pixels-per-lane / colour-in-LDS / checkpoint axes
            cur = re.sub(r'raster_wave_fwd_kernelILi1E(Li\d+E)Lb0ELb0EEEv10RasterArgsjjPfi', r'raster_wave_fwd_kernelI\1EEv10RasterArgsjj', cur)
            cur = re.sub(r'raster_wave_bwd_kernelILi1E(Li\d+ELi\d+ELb[01]E)', r'raster_wave_bwd_kernelI\1', cur)
            # projection_bwd_kernel before its per-pair inputs became a template policy: ONE instance <NEED_VIEW, SHDEG> served the
            # array and the row form, so both new instances <NEED_VIEW, SHDEG, ArrayPairs | RowPairs> are compared with it
            m = re.match(r'(.*projection_bwd_kernelILb[01]ELin?\d+E)(?:NS_\d+(ArrayPairs|RowPairs)E)?EEv', cur)
            if m:
                cur = m.group(1) + (' [' + m.group(2) + ']' if m.group(2) else '')
            out[cur] = []
        elif cur is not None and ln.strip():
            out[cur].append(re.sub(r'<[^>]*>', '<L>', ln.strip()))
    return out
A, B = kernels('/tmp/isa_a.txt'), kernels('/tmp/isa_b.txt')
base = lambda k: k.split(' [')[0]  # a new instance tagged ' [policy]' is compared with the old one without the tag
for k in sorted((set(A) - {base(k) for k in B}) | set(B)):
    if frag and frag not in k:
        continue
    a, b = A.get(k, A.get(base(k))), B.get(k)
    if a is None or b is None:
        print(('ONLY-OLD ' if b is None else 'ONLY-NEW ') + k[:150]); continue
    print(('SAME     ' if a == b else f'DIFF {len(a)}->{len(b)} ') + k[:150])
PY
