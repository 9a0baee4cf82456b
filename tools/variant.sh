#!/bin/bash
# Study builds of libscde_hip.so with one kernel file compiled under extra -D flags (or from a git
# revision): tools/variant.sh FILE NAME "FLAGS" [NAME2 "FLAGS2" ...]; FILE is the kernel file to
# vary (kernels, unique, boot, ratio, or any other file of scde_amd/csrc, with or without
# .hip); FLAGS "@REV" builds FILE as of git revision REV.  Timing builds (results wrong by
# construction) are variants too: tools/variant.sh kernels kt3 "-DSCDE_KT_DIAG=3".  Writes
# var/libNAME.so (load with SCDE_LIB=var/libNAME.so).
# The compiler, its flags and the other objects come from scde_amd/csrc/Makefile.
set -e
cd "$(dirname "$0")/../scde_amd/csrc"
stem=$(basename "$1" .hip); shift
[[ -f $stem.hip ]] || { echo "variant.sh: no scde_amd/csrc/$stem.hip" >&2; exit 2; }
make -s
hipcc=$(make -s print-HIPCC); flags=$(make -s print-HIPFLAGS); arch=$(make -s print-ARCH)
objs=$(make -s print-OBJS | tr ' ' '\n' | grep -vx $stem.o | tr '\n' ' ')
mkdir -p ../../var
args=("$@")
for ((i = 0; i < ${#args[@]}; i += 2)); do
  f=${args[i+1]}; src=$stem.hip
  if [[ $f == @* ]]; then src=../../var/${stem}_${args[i]}.hip; git show ${f#@}:scde_amd/csrc/$stem.hip > $src; f=""; fi
  $hipcc $flags -I. $f -c $src -o ../../var/${stem}_${args[i]}.o &
done
wait
for ((i = 0; i < ${#args[@]}; i += 2)); do
  $hipcc -shared -fPIC --offload-arch=$arch -o ../../var/lib${args[i]}.so ../../var/${stem}_${args[i]}.o $objs
done
