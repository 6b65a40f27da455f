#!/bin/bash
# Build the library with the kernel units of the search path (search_fm.hip,
# search_text.hip, locate_sort.hip, patterns.hip, hits.hip)
# compiled under extra -D flags, for A/B runs (tools/ab_lib.sh, SAHARA_HIP_LIB):
# tools/build_variant.sh NAME -DFLAG ...
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
N=$1; shift
mkdir -p "$R/build/var" "$R/sahara_amd/lib/var"
make -C "$R" -s -j8 >/dev/null
var=""
KERNEL_UNITS="search_fm search_text locate_sort patterns hits"
for U in $KERNEL_UNITS; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-result "$@" -c "$R/sahara_amd/csrc/$U.hip" -o "$R/build/var/${U}_$N.o"
  var="$var $R/build/var/${U}_$N.o"
done
objs=$(ls "$R"/build/obj/*.o | grep -v $(for U in $KERNEL_UNITS; do echo "-e /$U.o\$"; done))
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs $var -o "$R/sahara_amd/lib/var/lib_$N.so" -lpthread
echo "$R/sahara_amd/lib/var/lib_$N.so"
