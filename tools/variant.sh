#!/bin/bash
# Build a variant of the library for an in-run A/B: tools/variant.sh <name> <file.hip> <extra hipcc flags...>  ->  variants/libssi_<name>.so
# (only <file.hip> is recompiled with the flags; the other objects are the in-tree ones).  Use with SSI_HIP_LIB=$PWD/variants/libssi_<name>.so
# <file.hip> is one of the Makefile's SRCS; the source list and the compile flags are the Makefile's (make print-SRCS / print-CXXFLAGS / ...).
# A flag read by an attention kernel file (attn_fwd.h, attn_bwd_dq.h, attn_bwd_dkv.h) goes on their translation unit, attention_mfma.hip;
# one read by a bf16 GEMM kernel file (gemm_mfma.h, gemm_wg8.h, gemm_nt4.h) on theirs, gemm_mfma.hip; one read by gemm_skinny.h (the skinny
# GEMMs' shared merge, epilogues and host frame) on whichever of its two units is being varied, gemm_skinny.hip or gemm_wq8.hip.
set -e
name=$1; src=$2; shift 2
cd "$(dirname "$0")/../speech-integration_amd/csrc"
make -s -j8 >/dev/null
hipcc=$(make -s print-HIPCC); arch=$(make -s print-ARCH); srcs=$(make -s print-SRCS)
case " $srcs " in *" $src "*) ;; *) echo "variant.sh: $src is not one of: $srcs" >&2; exit 2;; esac
mkdir -p ../../variants
$hipcc $(make -s print-CXXFLAGS) "$@" -c $src -o ../../variants/$name.o
objs=""
for f in $srcs; do
  if [ "$f" = "$src" ]; then objs="$objs ../../variants/$name.o"; else objs="$objs ${f%.hip}.o"; fi
done
$hipcc --offload-arch=$arch -shared -fPIC -o ../../variants/libssi_$name.so $objs
echo "variants/libssi_$name.so"
