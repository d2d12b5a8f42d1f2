// render_knobs.h -- fused renderer: every build-time constant of render.hip, with the measurements that chose its default.
// Each is overridden with -DNAME=value on the compile line (tools/build_variant.sh, tools/kernel_resources.sh and tools/render_isa_sha.sh
// pass such flags through).  "read by": the function that uses it (the opening comment of render.hip says which file holds what);
// "set by": the tool that builds variants of it; none = only by hand.
#ifndef SN_RENDER_KNOBS_H
#define SN_RENDER_KNOBS_H

// ---- gathers ------------------------------------------------------------------------------------
// read by: half_wave_swap.  set by: tools/xswap_ab.sh
#ifndef SN_XSWAP_MODE
#define SN_XSWAP_MODE 0      // which lanes trade the two x-corners of a cell (A/B, tools/xswap_ab.sh, profiles/r06/xswap_ab.txt; all bit-identical): 0 = the wave's
                             // halves (v_permlane32_swap; 6.21-6.27 ms); 1 = neighbours (lanes 2i, 2i+1: both corners of a ray in ONE quad of the address unit, 13 %
                             // fewer quad-line pairs but 40 % more distinct lines per instruction and a select per swap: 6.43-6.45 ms); 2 = 16-lane rows
                             // (v_permlane16_swap: 6.19-6.20 ms, inside the noise of the default)
#endif
// read by: parity_level.  set by: none
#ifndef SN_PARITY_FIRST
#define SN_PARITY_FIRST 12   // first hashed level issued by parity: 9 / 11 / 12 / 13 / 14 measured (profiles/r10/README.md); levels 7-11 sit at the 8-line floor of
                             // the address unit already (tools/gather_parity_table.py) and the exchange costs ~18 vector instructions per level
#endif
// read by: parity_level.  set by: none
#ifndef SN_PARITY_AXES
#define SN_PARITY_AXES 2     // 2 = y and z, 1 = z only
#endif
// read by: swap_if, swap_if4.  set by: none
#ifndef SN_PARITY_UNDO
#define SN_PARITY_UNDO 1     // how odd lanes trade two registers (address terms at issue, landed values at the blend): 0 = two selects per pair (26 vector instructions per
                             // level: slower than the canonical order, profiles/r10/undo_by_selects_ab.json), 1 = one v_swap_b32 per pair with the odd lanes as the exec mask (18)
#endif
// read by: final_stage_rays (its FinalSpans choice), fp32 tables.  set by: none
#ifndef SN_FINAL_SPANS_LT
#define SN_FINAL_SPANS_LT 4    // linear-tail instantiation: 64 weight-accumulated hidden values per lane live through the march -> short span 0
#endif
// read by: final_stage_rays (its FinalSpans choice), fp16 tables.  set by: none
#ifndef SN_FINAL_SPANS_LT_H
#define SN_FINAL_SPANS_LT_H 4  // the same for fp16 tables
#endif

// ---- proposal stage -----------------------------------------------------------------------------
// read by: k_prop_stage (GROUP of encode_levels), fp32 tables.  set by: none
#ifndef SN_PROP_GROUP
#define SN_PROP_GROUP 2      // proposal stage: levels gathered in groups of 2 + 2 + 1.  History: all 5 at once spilled at 128 VGPRs; 3 + 2 fitted
                             // (4.70 -> 4.55 ms); 2 + 2 + 1 fits 96 VGPRs = 5 waves per SIMD instead of 4 (SN_PROP_WAVES): [128,64,32] 4.53 -> 4.44 ms fp32
#endif
// read by: k_prop_stage (GROUP of encode_levels), fp16 tables.  set by: none
#ifndef SN_PROP_GROUP_H
#define SN_PROP_GROUP_H 2    // the same for fp16 tables (78 VGPRs): 4.10 -> 3.98 ms
#endif
// read by: k_prop_stage, pass 2.  set by: none
#ifndef SN_PROP_PB
#define SN_PROP_PB 4         // cdf entries per block of the sample_pdf merge (pass 2 of the proposal stage); 8: same, 16: slower (select chains)
#endif
// read by: k_prop_stage's launch bounds (UN = 1).  set by: none
#ifndef SN_PROP_WAVES
#define SN_PROP_WAVES 5      // waves per SIMD the proposal stage is compiled for (register budget 512 / N in steps of 8: 96 VGPRs); the
                             // stage is bound by each wave's dependent chain, so a fifth wave buys 3-4 % (profiles/r02/ab_round2_experiments.txt)
#endif
// read by: k_prop_stage (GROUP of encode_levels_multi).  set by: none
#ifndef SN_PROP_GROUP_U2
#define SN_PROP_GROUP_U2 1   // levels per gather group of the two-samples-at-once instantiation (x 2 positions)
#endif
// read by: k_prop_stage's launch bounds (UN = 2).  set by: none
#ifndef SN_PROP_WAVES_U2
#define SN_PROP_WAVES_U2 3   // the two-samples-at-once instantiation (UN = 2): 168 VGPRs
#endif

// ---- last stage ---------------------------------------------------------------------------------
// read by: plan_chunk (host).  set by: none
#ifndef SN_FINAL_SP_MIN_BLOCKS
#define SN_FINAL_SP_MIN_BLOCKS 256u    // the several-lanes-per-ray last stage takes fewer samples per lane until the launch has this many workgroups
                                       // (round 6, same box: 512 / 1024 are 3-8 % slower from 4096 to 16 384 rays -- one workgroup per CU is this kernel's optimum)
#endif
// read by: k_final_stage's launch bounds.  set by: none
#ifndef SN_FINAL_WAVES
#define SN_FINAL_WAVES 2     // waves per SIMD k_final_stage is compiled for (register budget); experiments only
#endif

#endif  // SN_RENDER_KNOBS_H
