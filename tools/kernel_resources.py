#!/usr/bin/env python
"""Registers, scratch and LDS of every kernel of the hot files, from the compiler's own metadata (hipcc -S for gfx950; no
GPU needed).  Occupancy on CDNA4 is decided here: 512 VGPRs per SIMD lane in steps of 8 (<= 128: four waves per SIMD,
<= 168: three, <= 256: two), and a kernel that spills (scratch > 0) pays a vmcnt(0) per reload.  Round 5 lost 20 us of
the SH forward and 190 us of the fixed-point per-gaussian backward to register counts that had drifted across such a
step unnoticed; tests/test_kernel_budgets.py now holds the kernels below to their budgets.

    python tools/kernel_resources.py [file.hip ...]        # table on stdout
    python tools/kernel_resources.py --diff OTHER_CSRC_DIR [--show] [file.hip ...]
        # a refactor's proof: the assembly of every kernel of this tree against another csrc directory (default: every
        # file of SRCS in the Makefile); exit status 1 if any kernel differs
"""
import difflib
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / 'taichi_splatting_amd' / 'csrc'
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fno-fast-math', '-fno-slp-vectorize', '-S', '--cuda-device-only']
DEFAULT = ['raster_bwd_scan.hip', 'raster_fast.hip', 'sh.hip', 'gaussian_bwd.hip', 'projection.hip', 'mapper.hip']
FIELDS = (('vgpr', 'next_free_vgpr'), ('sgpr', 'next_free_sgpr'), ('scratch', 'private_segment_fixed_size'),
          ('lds', 'group_segment_fixed_size'))


def demangle(names):
  try:
    out = subprocess.run(['c++filt'], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return out.splitlines()
  except Exception:
    return names


def kernels(path):
  """{demangled kernel name: dict(vgpr, sgpr, scratch, lds, asm)} of one .hip file; asm = the lines from the kernel's
  `.type NAME,@function` to its `.Lfunc_end` (body and descriptor), without those that name the per-translation-unit
  __hip_cuid_ symbol.  A device function the compiler did not inline is listed like a kernel, without resources."""
  asm = subprocess.run(['/opt/rocm/bin/hipcc', *FLAGS, str(path), '-o', '-'], capture_output=True, text=True)
  if asm.returncode != 0:
    raise RuntimeError(f"hipcc -S {path}: {asm.stderr[-2000:]}")
  out, cur = {}, None
  for line in asm.stdout.splitlines():
    m = re.match(r'\s*\.type\s+(\S+),@function', line)
    if m:
      cur = dict(name=m.group(1), asm=[])
    if cur is None or '__hip_cuid_' in line:
      continue
    cur['asm'].append(line)
    for key, field in FIELDS:
      m = re.match(rf'\s*\.amdhsa_{field}\s+(\d+)', line)
      if m:
        cur[key] = int(m.group(1))
    if line.startswith('.Lfunc_end'):
      out[cur.pop('name')] = cur
      cur = None
  names = list(out)
  return {d: out[n] for n, d in zip(names, demangle(names))}


def resources(path):
  """{demangled kernel name: dict(vgpr, sgpr, scratch, lds)} of one .hip file"""
  return {name: {key: v for key, v in k.items() if key != 'asm'} for name, k in kernels(path).items() if 'vgpr' in k}


def waves_per_simd(vgpr):
  return min(8, 512 // (((vgpr + 7) // 8) * 8))


def short(name):
  return re.sub(r'\(.*', '', name).replace('void ', '')


def instructions(asm):
  return sum(1 for line in asm if re.match(r'\s+[a-z]\w*(\s|$)', line) and not line.lstrip().startswith('.'))


def diff(other, names, show):
  """compare every kernel of the named files between this tree and the csrc directory `other`; True if all are identical"""
  names = names or re.search(r'^SRCS\s*=\s*(.*)$', (SRC / 'Makefile').read_text(), re.M).group(1).split()
  with ThreadPoolExecutor(8) as pool:        # two trees per worker step: at most 16 compiles at a time
    tables = list(pool.map(lambda f: (kernels(SRC / f), kernels(Path(other) / f)), names))
  same = True
  for f, (new, old) in zip(names, tables):
    print(f"== {f}")
    for name in sorted(set(new) | set(old)):
      a, b = old.get(name), new.get(name)
      if a and b and a['asm'] == b['asm']:
        print(f"  {short(name)[:86]:86s} identical")
        continue
      same = False
      for side, k in (('other', a), ('this', b)):
        print(f"  {short(name)[:86]:86s} {side:5s} " + ("absent" if k is None else f"instructions {instructions(k['asm']):5d}  "
              f"vgpr {k.get('vgpr', 0):4d}  sgpr {k.get('sgpr', 0):3d}  scratch {k.get('scratch', 0):4d}  lds {k.get('lds', 0):6d}"))
      if show and a and b:
        print("\n".join(difflib.unified_diff(a['asm'], b['asm'], 'other', 'this', lineterm='', n=2)))
  return same


def main():
  args = sys.argv[1:]
  if '--diff' in args:
    at = args.index('--diff')
    other = args[at + 1]
    del args[at:at + 2]
    show = '--show' in args
    sys.exit(0 if diff(other, [a for a in args if a != '--show'], show) else 1)
  files = [SRC / f for f in (args or DEFAULT)]
  with ThreadPoolExecutor(len(files)) as pool:
    tables = list(pool.map(resources, files))
  for f, table in zip(files, tables):
    print(f"== {f.name}")
    for name, r in sorted(table.items()):
      print(f"  {short(name)[:86]:86s} vgpr {r.get('vgpr', 0):4d} ({waves_per_simd(r.get('vgpr', 1))} waves/SIMD)  sgpr {r.get('sgpr', 0):3d}  scratch {r.get('scratch', 0):4d}  lds {r.get('lds', 0):6d}")


if __name__ == '__main__':
  main()
