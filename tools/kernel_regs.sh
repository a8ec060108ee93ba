#!/bin/bash
# Register / scratch use of every kernel in one source file: tools/kernel_regs.sh gemm_mfma.hip [extra flags] (no GPU needed; the Makefile's
# compile flags; the attention kernels of attn_fwd.h, attn_bwd_dq.h and attn_bwd_dkv.h: attention_mfma.hip, their translation unit; the bf16
# GEMM kernels of gemm_wg8.h and gemm_nt4.h: gemm_mfma.hip; the skinny GEMMs' shared gemm_skinny.h: gemm_skinny.hip or gemm_wq8.hip, whose
# kernel is being looked at)
B=/opt/rocm/lib/llvm/bin; src=$1; shift
cd "$(dirname "$0")/../speech-integration_amd/csrc"
$(make -s print-HIPCC) $(make -s print-CXXFLAGS) --cuda-device-only "$@" -c $src -o /tmp/kr.co
$B/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=/tmp/kr.co --output=/tmp/kr.elf
$B/llvm-readelf --notes /tmp/kr.elf | grep -E "^\s+\.name:|private_segment_fixed_size|\.vgpr_count|agpr_count|vgpr_spill|sgpr_spill" | paste - - - - - - | sed 's/ \+/ /g; s/_ZN12_GLOBAL__N_1//'
