#!/bin/bash
# Diagnostic: builds build/exp_<name>/libvolren_amd.so with extra compiler flags (e.g. -DVR_WAVES_PER_SIMD=5 -DVR_NSLOT=126); run with
# VOLREN_AMD_LIB=build/exp_<name>/libvolren_amd.so.
#   usage: [VARIANTS="0 1"] bash tests/tools_build_variant.sh <name> <flags...>
#   VARIANTS: the path-tracing kernel variants to recompile with the flags (every build of them: bit-exact, tolerance mode, wide); everything else is taken from
#   the default build in build/ (run `make` first).  Without VARIANTS every object is recompiled with the flags (for the ones that reach the launch code or the
#   host: VR_C_STRIDE, the layout switches of vr_scene.h).
# The objects, their flags and the link are the Makefile's (OBJDIR, EXTRA): nothing is listed here.
set -e
name=$1; shift
out=build/exp_$name; mkdir -p $out
rm -f $out/*.o
if [ -n "$VARIANTS" ]; then
  cp -p build/*.o $out/                      # with their time stamps: make takes them as built
  for v in $VARIANTS; do rm -f $out/vr_pathtrace_$v.o $out/vr_ptfast_$v.o $out/vr_ptwide_$v.o $out/vr_ptwf_$v.o; done
fi
make -j${MAX_JOBS:-8} OBJDIR=$out EXTRA="$*" $out/libvolren_amd.so > $out/make.log 2>&1 || { tail -20 $out/make.log; exit 1; }
for v in ${VARIANTS:-0 1 2 3 4}; do grep -h -A8 "pathtrace_kernel" $out/vr_pathtrace_$v.resources.txt | grep -E "Function Name|VGPRs:|SGPRs Spill|VGPRs Spill|ScratchSize" | sed 's/.*remark: [^ ]* *//; s/ \[-R.*//' | paste - - - - - | sed "s/^/v$v: /"; done
