#!/bin/bash
# Study builds of libscde_hip.so with kernels.hip compiled under extra -D flags (or from a git
# revision): tools/variant.sh NAME "FLAGS" [NAME2 "FLAGS2" ...]; FLAGS "@REV" builds kernels.hip as
# of git revision REV.  Timing builds (results wrong by construction) are variants too:
# tools/variant.sh kt3 "-DSCDE_KT_DIAG=3".  Writes var/libNAME.so (load with SCDE_LIB=var/libNAME.so).
# The compiler, its flags and the other objects come from scde_amd/csrc/Makefile.
set -e
cd "$(dirname "$0")/../scde_amd/csrc"
make -s
hipcc=$(make -s print-HIPCC); flags=$(make -s print-HIPFLAGS); arch=$(make -s print-ARCH)
objs=$(make -s print-OBJS | tr ' ' '\n' | grep -vx kernels.o | tr '\n' ' ')
mkdir -p ../../var
args=("$@")
for ((i = 0; i < ${#args[@]}; i += 2)); do
  f=${args[i+1]}; src=kernels.hip
  if [[ $f == @* ]]; then src=../../var/kernels_${args[i]}.hip; git show ${f#@}:scde_amd/csrc/kernels.hip > $src; f=""; fi
  $hipcc $flags -I. $f -c $src -o ../../var/kernels_${args[i]}.o &
done
wait
for ((i = 0; i < ${#args[@]}; i += 2)); do
  $hipcc -shared -fPIC --offload-arch=$arch -o ../../var/lib${args[i]}.so ../../var/kernels_${args[i]}.o $objs
done
