#!/bin/bash
# Build a variant libvgpa_hip.so for A/B runs inside ONE GPU session: the product objects, with the sources that take measurement knobs
# (attention_hd128.hip: -DATTN128_W1_MIN_KEYS=; lora.hip: -DLORA_DOWN_NS=, -DLORA_DOWN_DMA=, -DLORA_DOWN_DMA_NCB=, -DLORA_GRAD_WGS=) recompiled
# with the extra -D flags, plus the GEMM probe of tools/variants/ (-DVGPA_VARIANTS):
#   tools/build_variant.sh NAME [-DFOO ...]   ->  var/lib_NAME.so   (select with: VGPA_LIB=$PWD/var/lib_NAME.so python tools/attn128_time.py;
#   the product library videogpa_amd/csrc/libvgpa_hip.so is never overwritten.  var/ is git-ignored)
set -e
cd "$(dirname "$0")/.."
name=$1; shift
python -m videogpa_amd.build >/dev/null
mkdir -p var /tmp/vobj_$name
for src in videogpa_amd/csrc/attention_hd128.hip videogpa_amd/csrc/lora.hip tools/variants/gemm_w1.hip; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-mfma-vgpr-form=1 -munsafe-fp-atomics -fno-slp-vectorize -Wno-unused-function \
    -I include -I videogpa_amd/csrc -I tools/variants -DVGPA_VARIANTS "$@" -c $src -o /tmp/vobj_$name/$(basename $src .hip).o
done
objs=$(ls videogpa_amd/csrc/_obj/*.o | grep -v "/attention_hd128.o\|/lora.o\|/gemm_w1.o")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs /tmp/vobj_$name/*.o -o var/lib_$name.so
echo "built var/lib_$name.so"
