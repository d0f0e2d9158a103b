#!/bin/bash
# Build an instrumented development variant of libmi355_splat.so into tools/variants/lib<name>.so: the product sources
# and flags (SRCS and CXXFLAGS of taichi_splatting_amd/csrc/Makefile) plus the extra hipcc flags given here.  The three
# instruments measure the product kernels without changing their results, and are the only supported variants:
#   tools/build_variant.sh stats     -DMS_SCAN_STATS=1     (ms_debug_scan_stats:  work counters of the raster backward)
#   tools/build_variant.sh phases    -DMS_SCAN_PHASES=1    (ms_debug_scan_phases: a backward wave's cycles per phase)
#   tools/build_variant.sh fwdphases -DMS_FWD_PHASES=1     (ms_debug_fwd_phases:  a forward wave's cycles per phase)
# Select it at run time with MS_SPLAT_LIB=tools/variants/lib<name>.so (taichi_splatting_amd/_lib.py).
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
src=$root/taichi_splatting_amd/csrc
out=$root/tools/variants/obj_$name
makevar() { make -s -C "$src" --no-print-directory --eval='print-%: ; @echo $($*)' "print-$1"; }
hipcc=$(makevar HIPCC); flags=$(makevar CXXFLAGS); srcs=$(makevar SRCS)
mkdir -p "$out"
pids=()
for f in $srcs; do
  $hipcc $flags "$@" -c "$src/$f" -o "$out/${f%.hip}.o" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
$hipcc --offload-arch=$(makevar ARCH) -shared -fPIC -o "$root/tools/variants/lib$name.so" "$out"/*.o
rm -rf "$out"
echo "built tools/variants/lib$name.so"
