#!/usr/bin/env bash
# Dumps the gfx950 ISA + resource usage of the library's kernels into /tmp/lmi_isa (developer aid).
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
out="${1:-/tmp/lmi_isa}"
mkdir -p "$out" && cd "$out"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I"${here}/../../include" -I"${here}" \
  ${LMI_EXTRA_FLAGS:-} -c "${here}/lmi_hip.hip" -o x.o -save-temps -Rpass-analysis=kernel-resource-usage 2> usage.txt || { cat usage.txt; exit 1; }
S=lmi_hip-hip-amdgcn-amd-amdhsa-gfx950.s
awk '/^_ZN3lmi11scan_kernelENS_10ScanParamsE:/,/s_endpgm/' $S > scan.s
grep -A12 "Function Name: _ZN3lmi11scan_kernel" usage.txt | grep -E "VGPRs:|Spill|Occupancy|LDS Size|SGPRs:" | sed 's/remark: [^ ]* //'
echo "mfma $(grep -c v_mfma scan.s)  glds $(grep -c global_load_lds scan.s)  scratch $(grep -c scratch_ scan.s)  lines $(wc -l < scan.s)"
# lmi_knn_hamming's score kernel (16-byte form): its inner loop is 256 xor + 256 bcnt per chunk of 8 words x 32 queries
awk '/^_ZN3lmi20hamming_score_kernelILb1EEEvPKjxiS2_iiiPfx:/,/s_endpgm/' $S > hamming.s
grep -A12 "Function Name: _ZN3lmi20hamming_score_kernelILb1" usage.txt | grep -E "VGPRs:|Spill|Occupancy|ScratchSize|SGPRs:" | sed 's/remark: [^ ]* //'
echo "hamming: xor $(grep -c v_xor_b32 hamming.s)  bcnt $(grep -c v_bcnt_u32_b32 hamming.s)  s_load $(grep -c s_load_dword hamming.s)  scratch $(grep -c scratch_ hamming.s)  lines $(wc -l < hamming.s)"
# lmi_knn_rerank's score kernel (16-byte form; IP, then L2): per chunk of 32 words the 32 links in ascending order -- IP: one v_fma_f32
# and 31 v_fmac_f32 (+ 1 in the loop of the last, partial chunk), the query operand of each an SGPR; L2: 32 v_pk_fma_f32, the links of
# s and xn of one element side by side; the 8 global_load_dwordx4 of the next chunk before them; no scratch
# lmi_sketch's kernel (float rows, four tiles a wave, 16-byte loads): per 32-link chunk 128 v_mfma_f32_32x32x2_f32 and 32 v_sub_f32 as
# in project_kernel; behind the loop 128 v_cmp_gt_f32 (16 per tile and row block), one v_permlane32_swap per tile (beside the 32 of
# dense_load_b) and one global_store_dwordx4; the only ds_writes stage the mean and the thresholds (no transpose); no scratch
awk '/^_ZN3lmi13sketch_kernelIfLi4ELb1EEE[^:]*:/,/s_endpgm/' $S > sketch.s
grep -A12 "Function Name: _ZN3lmi13sketch_kernelIfLi4ELb1EEE" usage.txt | grep -E "VGPRs:|Spill|Occupancy|ScratchSize|LDS Size|SGPRs:" | sed 's/remark: [^ ]* //'
echo "sketch: mfma $(grep -c v_mfma_f32_32x32x2 sketch.s)  cmp_gt $(grep -c v_cmp_gt_f32 sketch.s)  permlane32_swap $(grep -c v_permlane32_swap sketch.s)  store_dwordx4 $(grep -c global_store_dwordx4 sketch.s)  ds_write $(grep -cE 'ds_write|ds_store' sketch.s)  scratch $(grep -c scratch_ sketch.s)  lines $(wc -l < sketch.s)"
for m in 0 1; do
  awk "/^_ZN3lmi19rerank_score_kernelILb1ELb${m}EEE[^:]*:/,/s_endpgm/" $S > rerank$m.s
  grep -A12 "Function Name: _ZN3lmi19rerank_score_kernelILb1ELb${m}EEE" usage.txt | grep -E "VGPRs:|Spill|Occupancy|ScratchSize|LDS Size|SGPRs:" | sed 's/remark: [^ ]* //'
  echo "rerank L2=$m: fmac $(grep -c v_fmac_f32 rerank$m.s)  of them with an SGPR $(grep -cE 'v_fmac_f32(_e32)? v[0-9]+, s[0-9]+' rerank$m.s)  pk_fma $(grep -c v_pk_fma_f32 rerank$m.s)  v_fma/mul/add_f32 $(grep -cE 'v_(fma|mul|add)_f32' rerank$m.s)  dwordx4 $(grep -c global_load_dwordx4 rerank$m.s)  s_load $(grep -c s_load_dword rerank$m.s)  scratch $(grep -c scratch_ rerank$m.s)  lines $(wc -l < rerank$m.s)"
done
