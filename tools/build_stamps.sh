#!/bin/bash
# Developer tool: experiment build of the library with in-kernel time stamps (-DGMMVI_ME_STAMPS) as
# gmmvi_amd/libgmmvi_hip_stamps.so; use it with GMMVI_HIP_LIB=gmmvi_amd/libgmmvi_hip_stamps.so (tools/pk_stamps.py).
# The one-sample and the packed sweep kernel write the same device-side stamp buffers, so under that define density_reg.hip
# holds the text of density_pk.hip too and replaces both objects.
set -e
cd "$(dirname "$0")/../gmmvi_amd/csrc"
make -j8 >/dev/null
mkdir -p build_stamps
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I../../include -Wno-unused-function -ffp-contract=fast \
    -DGMMVI_ME_STAMPS $EXTRA_DEFS -c density_reg.hip -o build_stamps/density_reg.o
objs=$(ls build/*.o | grep -v -e density_reg.o -e density_pk.o)
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib $objs build_stamps/density_reg.o \
    -o ../libgmmvi_hip_stamps.so
echo built gmmvi_amd/libgmmvi_hip_stamps.so
