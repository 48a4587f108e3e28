// fpv_derive.h - host-side narrowing of fpv_params_t (double) to the kernel constants FpvK (fp32).
//
// Everything that can be folded on the host in double precision is folded here, once per
// fpv_create/fpv_set_params, so the per-lane fp32 arithmetic starts from correctly rounded
// constants:
//   * the thrust cubic over throttle PERCENT (components.py:136, x = 100(a+1)/2) is re-expanded
//     around the stick value a (x = 50a + 50): same polynomial, but |a| <= 1 keeps the fp32 Horner
//     terms the size of the result instead of cancelling ~90 N against ~-36 N;
//   * 0.5*rho*Cd*A/m per body axis (kinematics.py:36 followed by components.py:243);
//   * deg/s -> half-angle per step, 0.5 * pi/180 * dt (kinematics.py:29).
#pragma once

#include <math.h>
#include <string.h>

#include "../../include/fpv_abi.h"
#include "fpv_math.h"

// The per-drone part of the narrowing (include/fpv_abi.h "Per-drone physics"): the FPV_PHYS_ROWS constants of ONE parameter set
// `in` (FPV_PHYS_INPUTS doubles: mass, c3 c2 c1 c0, Cd x y z, rates_transition_rate, thrust_transition_rate) on the uniform
// parameters of `P` (max_rates, air density, cross sections, ground spring / damping).  fpv_derive_constants calls it with P's own
// values, fpv_physics_derive once per drone: a drone's table column IS the constants of a handle built with its parameters.
static inline void fpv_derive_physics_rows(const fpv_params_t* P, const double in[FPV_PHYS_INPUTS], float row[FPV_PHYS_ROWS])
{
    const double mass = in[FPV_PHYS_IN_MASS], kr = in[FPV_PHYS_IN_RATES_LAG], kt = in[FPV_PHYS_IN_THRUST_LAG];
    const double c3 = in[FPV_PHYS_IN_C3], c2 = in[FPV_PHYS_IN_C2], c1 = in[FPV_PHYS_IN_C1], c0 = in[FPV_PHYS_IN_C0];
    const double h = 50.0;   // x = h*a + h
    row[FPV_PHYS_RATE_LIM] = (float)(P->max_rates * kr);
    row[FPV_PHYS_OMKR] = (float)(1.0 - kr);
    row[FPV_PHYS_OMKT] = (float)(1.0 - kt);
    row[FPV_PHYS_DK3] = (float)(kt * (c3 * h * h * h));
    row[FPV_PHYS_DK2] = (float)(kt * (3 * c3 * h * h * h + c2 * h * h));
    row[FPV_PHYS_DK1] = (float)(kt * (3 * c3 * h * h * h + 2 * c2 * h * h + c1 * h));
    row[FPV_PHYS_DK0] = (float)(kt * (c3 * h * h * h + c2 * h * h + c1 * h + c0));
    for (int i = 0; i < 3; ++i)
        row[FPV_PHYS_KDRAG_X + i] = (float)(0.5 * in[FPV_PHYS_IN_CD_X + i] * P->air_density * P->cross_section_areas[i] / mass);
    row[FPV_PHYS_INV_MASS] = (float)(1.0 / mass);
    row[FPV_PHYS_GROUND_K_M] = (float)(P->ground_spring / mass);
    row[FPV_PHYS_GROUND_C_M] = (float)(P->ground_damping / mass);
}

// P's own parameter set as the inputs of fpv_derive_physics_rows
static inline void fpv_physics_base_inputs(const fpv_params_t* P, double in[FPV_PHYS_INPUTS])
{
    in[FPV_PHYS_IN_MASS] = P->mass;
    for (int i = 0; i < 4; ++i) in[FPV_PHYS_IN_C3 + i] = P->thrust_poly[i];
    for (int i = 0; i < 3; ++i) in[FPV_PHYS_IN_CD_X + i] = P->drag_coefficients[i];
    in[FPV_PHYS_IN_RATES_LAG] = P->rates_transition_rate;
    in[FPV_PHYS_IN_THRUST_LAG] = P->thrust_transition_rate;
}

// Returns 0 or an FPV_E* code; *why receives a static message on failure.
static inline int fpv_derive_constants(const fpv_params_t* P, FpvK* K, const char** why)
{
    *why = "";
    if (P->struct_size != sizeof(fpv_params_t)) { *why = "fpv_params_t.struct_size does not match this library"; return FPV_EINVAL; }
    if (P->mode != FPV_MODE_DRONE && P->mode != FPV_MODE_RACER) { *why = "unknown mode"; return FPV_EINVAL; }
    if ((P->flags & FPV_FLAG_FP16_STATE) && P->mode != FPV_MODE_DRONE) { *why = "FPV_FLAG_FP16_STATE is a drone-mode layout"; return FPV_EINVAL; }
    if ((P->flags & FPV_FLAG_STICK_NOISE) && (P->mode != FPV_MODE_DRONE || (P->flags & FPV_FLAG_FP16_STATE))) { *why = "FPV_FLAG_STICK_NOISE needs drone mode with fp32 state"; return FPV_EINVAL; }
    if ((P->flags & FPV_FLAG_STICK_NOISE) && !(P->noise_transition > 0 && P->noise_transition <= 1)) { *why = "noise_transition must be in (0, 1]"; return FPV_EPARAM; }
    if ((P->flags & FPV_FLAG_RESET_JITTER) && P->mode != FPV_MODE_DRONE) { *why = "FPV_FLAG_RESET_JITTER is a drone-mode reset source (the Racer resets to its zero state)"; return FPV_EINVAL; }
    if (!(P->dt > 0) || !isfinite(P->dt)) { *why = "dt must be positive and finite"; return FPV_EPARAM; }
    if (!(P->mass > 0)) { *why = "mass must be positive"; return FPV_EPARAM; }
    if (!(P->max_rates >= 0) || !isfinite(P->max_rates)) { *why = "max_rates must be finite and >= 0"; return FPV_EPARAM; }
    if (P->mode == FPV_MODE_RACER) {
        if (!(P->racer_mass > 0)) { *why = "racer_mass must be positive"; return FPV_EPARAM; }
        for (int i = 0; i < 3; ++i)
            if (!(P->racer_inertia[i] > 0)) { *why = "racer_inertia must be positive"; return FPV_EPARAM; }
        if (P->racer_pid_variant > 1) { *why = "racer_pid_variant must be 0 (racer_drone_test.PID) or 1 (components.PID)"; return FPV_EINVAL; }
        if (P->racer_pid_variant == 1 && (!(P->pid_integral_clip >= 0) || !(P->pid_min_output <= P->pid_max_output)
                                          || !(P->pid_derivative_transition_rate >= 0 && P->pid_derivative_transition_rate <= 1))) {
            *why = "components.PID constants: integral_clip >= 0, min_output <= max_output, derivative_transition_rate in [0, 1]";
            return FPV_EPARAM;
        }
    }
    const double qn = sqrt(P->init_quat[0] * P->init_quat[0] + P->init_quat[1] * P->init_quat[1] +
                           P->init_quat[2] * P->init_quat[2] + P->init_quat[3] * P->init_quat[3]);
    if (!(fabs(qn - 1.0) < 1e-6)) { *why = "init_quat must be a unit quaternion"; return FPV_EPARAM; }

    memset(K, 0, sizeof(*K));
    K->dt = (float)P->dt;
    K->max_rates = (float)P->max_rates;
    K->kr = (float)P->rates_transition_rate;
    K->kt = (float)P->thrust_transition_rate;
    const double c3 = P->thrust_poly[0], c2 = P->thrust_poly[1], c1 = P->thrust_poly[2], c0 = P->thrust_poly[3];
    const double h = 50.0;   // x = h*a + h
    K->d3 = (float)(c3 * h * h * h);
    K->d2 = (float)(3 * c3 * h * h * h + c2 * h * h);
    K->d1 = (float)(3 * c3 * h * h * h + 2 * c2 * h * h + c1 * h);
    K->d0 = (float)(c3 * h * h * h + c2 * h * h + c1 * h + c0);
    {   // everything a physics table can replace per drone, by the function that fills the table
        double in[FPV_PHYS_INPUTS];
        float row[FPV_PHYS_ROWS];
        fpv_physics_base_inputs(P, in);
        fpv_derive_physics_rows(P, in, row);
        K->rate_lim = row[FPV_PHYS_RATE_LIM];
        K->rate_gain = -K->rate_lim;
        K->omkr = row[FPV_PHYS_OMKR]; K->omkt = row[FPV_PHYS_OMKT];
        K->dk3 = row[FPV_PHYS_DK3]; K->dk2 = row[FPV_PHYS_DK2]; K->dk1 = row[FPV_PHYS_DK1]; K->dk0 = row[FPV_PHYS_DK0];
        for (int i = 0; i < 3; ++i) K->kdrag_m[i] = row[FPV_PHYS_KDRAG_X + i];
        K->inv_mass = row[FPV_PHYS_INV_MASS];
        K->ground_k_m = row[FPV_PHYS_GROUND_K_M]; K->ground_c_m = row[FPV_PHYS_GROUND_C_M];
    }
    K->g = (float)P->gravity;
    K->half_k = (float)(0.5 * (M_PI / 180.0) * P->dt);
    for (int m = 0; m < 4; ++m) { K->motor_x[m] = (float)P->motor_xy[m][0]; K->motor_y[m] = (float)P->motor_xy[m][1]; }
    {   // the reference's X frame after narrowing: (c,c) (-c,c) (-c,-c) (c,-c) in any order, one |c| bit for bit
        const float c = fabsf(K->motor_x[0]);
        bool square = c > 0.0f;
        int seen = 0;
        for (int m = 0; m < 4; ++m) {
            square = square && fabsf(K->motor_x[m]) == c && fabsf(K->motor_y[m]) == c;
            seen |= 1 << ((K->motor_x[m] < 0 ? 1 : 0) | (K->motor_y[m] < 0 ? 2 : 0));
        }
        K->motor_square = (square && seen == 15) ? 1u : 0u;
        K->motor_c = c;
    }
    for (int i = 0; i < 3; ++i) { K->p0[i] = (float)P->init_position[i]; K->v0[i] = (float)P->init_velocity[i]; K->goal[i] = (float)P->goal[i]; }
    for (int i = 0; i < 4; ++i) K->q0[i] = (float)(P->init_quat[i] / qn);
    K->ceiling = (float)P->ceiling;        // +inf stays +inf
    K->r_dt = (float)P->dt;
    K->r_inv_mass = (float)(1.0 / (P->racer_mass > 0 ? P->racer_mass : 1.0));
    K->r_damp = (float)P->racer_velocity_damping;
    K->r_ang_k = P->racer_omega_dt ? (float)P->dt : 1.0f;
    K->r_ang_k_d = P->racer_omega_dt ? P->dt : 1.0;
    // omega per STEP (as written) needs the float64 rate loop; omega*dt is well conditioned in fp32
    K->r_wide = P->racer_omega_dt ? 0u : 1u;
    K->r_pid_variant = P->racer_pid_variant;
    K->rd.dt = P->dt;
    K->rd.inv_dt = 1.0 / P->dt;
    for (int i = 0; i < 3; ++i) {
        K->rd.dt_over_I[i] = P->dt / (P->racer_inertia[i] > 0 ? P->racer_inertia[i] : 1.0);
        for (int j = 0; j < 3; ++j) K->rd.gain[i][j] = P->racer_pid[i][j];
    }
    K->rd.integral_clip = P->pid_integral_clip;
    K->rd.min_output = P->pid_min_output;
    K->rd.max_output = P->pid_max_output;
    K->rd.d_rate = P->pid_derivative_transition_rate;
    K->rd.om_d_rate = 1.0 - P->pid_derivative_transition_rate;
    K->rf.dt = (float)K->rd.dt; K->rf.inv_dt = (float)K->rd.inv_dt;
    for (int i = 0; i < 3; ++i) {
        K->rf.dt_over_I[i] = (float)K->rd.dt_over_I[i];
        for (int j = 0; j < 3; ++j) K->rf.gain[i][j] = (float)K->rd.gain[i][j];
    }
    K->rf.integral_clip = (float)K->rd.integral_clip; K->rf.min_output = (float)K->rd.min_output;
    K->rf.max_output = (float)K->rd.max_output; K->rf.d_rate = (float)K->rd.d_rate; K->rf.om_d_rate = (float)K->rd.om_d_rate;
    K->motor_radius = (float)P->motor_radius;
    double arm = 0.0;
    for (int m = 0; m < 4; ++m) arm = fmax(arm, sqrt(P->motor_xy[m][0] * P->motor_xy[m][0] + P->motor_xy[m][1] * P->motor_xy[m][1]));
    K->contact_reach = (float)(arm + fmax(P->motor_radius, 0.0) + 1e-3);
    K->noise.tau = (float)P->noise_transition;
    K->noise.omtau = (float)(1.0 - P->noise_transition);
    K->noise.gain = (float)P->noise_gain;
    K->noise.seed_lo = (uint32_t)P->noise_seed; K->noise.seed_hi = (uint32_t)(P->noise_seed >> 32);
    K->noise.id_lo = (uint32_t)P->drone_id_offset; K->noise.id_hi = (uint32_t)(P->drone_id_offset >> 32);
    K->flags = P->flags;
    // |rates| <= max_rates always (clip + convex low-pass from 0), so the largest half-angle of one
    // step is known here: up to 0.03 rad two series terms are exact to fp32, up to pi/4 the five-term
    // polynomials, beyond that the angle is reduced first (fpv_sincos3)
    const double half_max = 0.5 * (M_PI / 180.0) * P->dt * P->max_rates;
    K->angle_mode = half_max <= 0.03 ? FPV_ANGLE_TINY : half_max <= 0.78 ? FPV_ANGLE_SMALL : FPV_ANGLE_REDUCED;
    return FPV_OK;
}

// FPV_FLAG_RESET_JITTER: the three boxes narrowed to fp32 as lo and span = hi - lo (span in double, then narrowed: a box that
// straddles zero keeps its width); zeros without the flag.  Returns 0 or FPV_EPARAM (non-finite bound, lo > hi).
static inline int fpv_derive_reset_jitter(const fpv_params_t* P, FpvResetJitter* J, const char** why)
{
    *why = "";
    memset(J, 0, sizeof(*J));
    if (!(P->flags & FPV_FLAG_RESET_JITTER)) return FPV_OK;
    const double (*box[3])[3] = {P->reset_pos_range, P->reset_vel_range, P->reset_ypr_range_deg};
    for (int b = 0; b < 3; ++b)
        for (int c = 0; c < 3; ++c) {
            const double lo = box[b][0][c], hi = box[b][1][c];
            if (!isfinite(lo) || !isfinite(hi)) { *why = "reset_*_range bounds must be finite"; return FPV_EPARAM; }
            if (lo > hi) { *why = "reset_*_range: lo > hi"; return FPV_EPARAM; }
            J->lo[3 * b + c] = (float)lo;
            J->span[3 * b + c] = (float)(hi - lo);
        }
    J->seed_lo = (uint32_t)P->reset_seed; J->seed_hi = (uint32_t)(P->reset_seed >> 32);
    return FPV_OK;
}

// fpv_physics_derive (include/fpv_abi.h): the table columns of n parameter sets.  A NaN cell takes the base value.  Returns 0, or
// FPV_EPARAM with *bad = the first drone whose mass is not positive or that has an infinite cell.
static inline int fpv_derive_physics_table(const fpv_params_t* P, int64_t n, const double* inputs, float* out_rows, int64_t out_ld,
                                           int64_t* bad, const char** why)
{
    double base[FPV_PHYS_INPUTS];
    fpv_physics_base_inputs(P, base);
    for (int64_t i = 0; i < n; ++i) {
        double in[FPV_PHYS_INPUTS];
        float row[FPV_PHYS_ROWS];
        for (int c = 0; c < FPV_PHYS_INPUTS; ++c) {
            const double v = inputs ? inputs[i * FPV_PHYS_INPUTS + c] : base[c];
            in[c] = isnan(v) ? base[c] : v;
            if (isinf(in[c])) { *bad = i; *why = "a physics input is not finite"; return FPV_EPARAM; }
        }
        if (!(in[FPV_PHYS_IN_MASS] > 0)) { *bad = i; *why = "mass must be positive"; return FPV_EPARAM; }
        fpv_derive_physics_rows(P, in, row);
        for (int r = 0; r < FPV_PHYS_ROWS; ++r) out_rows[(int64_t)r * out_ld + i] = row[r];
    }
    return FPV_OK;
}

// fpv_physics_sample (include/fpv_abi.h): relative factors lo + (hi - lo) u on the base values, u = (w >> 8) * 2^-24 of a
// Philox4x32-7 word; key = seed, counter = (gid lo, gid hi ^ (block << 28), FPV_PHYS_SAMPLE_TAG, 0).  Block 0: words 0..3 = mass,
// motor strength (all four thrust coefficients; the range of the c3 column), rates lag, thrust lag; block 1: words 0..2 = Cd x y z.
#define FPV_PHYS_SAMPLE_TAG 0x53594850u      /* "PHYS" */
static inline void fpv_sample_physics_inputs(const fpv_params_t* P, uint64_t seed, uint64_t gid0, int64_t n, const double* ranges,
                                             double* out)
{
    double base[FPV_PHYS_INPUTS];
    fpv_physics_base_inputs(P, base);
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t gid = gid0 + (uint64_t)i;
        uint32_t w0[4], w1[4];
        fpv_philox4x32<FPV_NOISE_PHILOX_ROUNDS>((uint32_t)gid, (uint32_t)(gid >> 32), FPV_PHYS_SAMPLE_TAG, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w0);
        fpv_philox4x32<FPV_NOISE_PHILOX_ROUNDS>((uint32_t)gid, (uint32_t)(gid >> 32) ^ (1u << 28), FPV_PHYS_SAMPLE_TAG, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w1);
        double f[FPV_PHYS_INPUTS];
        const uint32_t word[FPV_PHYS_INPUTS] = {w0[0], w0[1], w0[1], w0[1], w0[1], w1[0], w1[1], w1[2], w0[2], w0[3]};
        for (int c = 0; c < FPV_PHYS_INPUTS; ++c) {
            const int rc = (c >= FPV_PHYS_IN_C3 && c <= FPV_PHYS_IN_C0) ? FPV_PHYS_IN_C3 : c;      // one factor for the whole cubic
            const double lo = ranges[2 * rc], hi = ranges[2 * rc + 1];
            f[c] = lo + (hi - lo) * ((double)(word[c] >> 8) * 0x1p-24);
            out[i * FPV_PHYS_INPUTS + c] = base[c] * f[c];
        }
    }
}
