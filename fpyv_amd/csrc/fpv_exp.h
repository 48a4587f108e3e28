// fpv_exp.h - the four build-time switches left for A/B builds (tools/ab_variants.py); the shipped library is built
// with neither defined.  Every other experiment hook of rounds 1-5 is closed and gone from the sources; what each
// one measured is in profiles/HISTORY.md.
#pragma once

// drones per workgroup of the step and k-step kernels (whole wave64s; the rotation's block, an XCD's share of a row)
#ifndef FPV_EXP_BLOCK
#define FPV_EXP_BLOCK 128
#endif

// occupancy bound of the single-step kernel: -DFPV_EXP_STEP_WAVES=N (or =MIN,MAX) waves per SIMD
#ifdef FPV_EXP_STEP_WAVES
#define FPV_EXP_STEP_ATTR __attribute__((amdgpu_waves_per_eu(FPV_EXP_STEP_WAVES)))
#else
#define FPV_EXP_STEP_ATTR
#endif

// table loads of the per-drone physics kernels (csrc/fpv_phys.hip): 0 = ordinary loads, 1 = with the streaming hint (shipped:
// 25.7 against 27.5 us per launch at 2^20 drones, 213 against 245 us at 2^23, rotated traversal; profiles/exp_phys_table_loads.log)
#ifndef FPV_EXP_PHYS_TABLE_NT
#define FPV_EXP_PHYS_TABLE_NT 1
#endif

// how a lane of the single-step gate kernel (csrc/fpv_gate.hip) reaches ITS gate's descriptor row: 1 = the workgroup stages the
// table into LDS at kernel entry (one barrier) and each lane reads its row by index (shipped: 28.70 against 28.80 us per launch at
// 2^20 drones, 221.1 against 227.2 us at 2^23 with the rotated traversal, 30.0 against 31.3 and 255.9 against 258.0 in the plain
// order; profiles/exp_gate_table_access.log), 0 = a per-lane gather from global memory once the word has arrived
#ifndef FPV_EXP_GATE_LDS
#define FPV_EXP_GATE_LDS 1
#endif
