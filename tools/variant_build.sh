#!/bin/bash
# builds a variant of the library with extra compiler flags next to the default one:
#   tools/variant_build.sh <name> <flags...>   ->  volxel_amd/libvolxel_hip_<name>.so  (use with VOLXEL_HIP_LIB=...)
set -e
name=$1; shift
cd "$(dirname "$0")/../volxel_amd/csrc"
tmp=$(mktemp -d)
objs=""
for u in vx_api vx_api_volume vx_api_view vx_api_segment vx_api_mesh; do   # the host layer's five units
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -Wall -Wno-unused-function "$@" -c $u.hip -o $tmp/$u.o &
  objs="$objs $tmp/$u.o"
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libvolxel_hip_$name.so $objs brick_builder.o dicom_reader.o -lpthread
rm -rf $tmp
ls -la ../libvolxel_hip_$name.so
