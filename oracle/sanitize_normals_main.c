/*
 * sanitize_normals_main.c — TEST INFRASTRUCTURE ONLY.  A stand-alone driver of oracle/wbc_ref.c's
 * per-foot ground normals for a host sanitizer build (`make -C oracle sanitize`): one stateful robot,
 * once per QP form, through 30 cycles of a mask-changing sequence on sloped ground, with the normals
 * replaced in mid-run and taken away for the last cycles.  Every input is fixed here; nothing is read.
 * The program exits 0 when every solve ended OK or INFEASIBLE with finite outputs (and at least one of
 * each form was OK); the sanitizer's own report ends it otherwise.
 */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "wbc_anymal_model.h"
#include "wbc_ref.h"

#define CYCLES 30

/* ten masks, three cycles each: every stance count, a change 7 -> 5 and 15 -> 13 that keeps rows */
static const int MASKS[10] = {15, 7, 5, 13, 15, 9, 6, 0, 15, 13};
static const double Q0[12] = {0.0, -0.4, 0.8, 0.0, 0.4, -0.8, 0.0, 0.4, -0.8, 0.0, -0.4, 0.8};
static const double FEET0[12] = {-0.506953, 0.31775, 0.0, 0.506953, 0.31775, 0.0, 0.506953, -0.31775, 0.0, -0.506953, -0.31775, 0.0};
static const double NORMALS[2][12] = {
    {0.20, -0.10, 0.95, -0.05, 0.30, 1.10, 0.0, 0.0, 0.7, -0.25, -0.15, 0.90},
    {-0.15, 0.05, 1.00, 0.10, 0.10, 0.80, 0.30, 0.0, 0.9, 0.0, 0.0, 1.0},
};

static int run(int method) {
    wbc_params pr;
    memset(&pr, 0, sizeof pr);
    pr.friction = 1.0; pr.loop_rate = 400.0; pr.max_torque = 80.0;
    pr.kp = 6000.0; pr.kp_z = 10000.0; pr.kd = 1800.0; pr.ki = 0.0;
    pr.kp_swing = 250.0; pr.kd_swing = 20.0; pr.slack_weight = 1000.0;
    pr.initial_reference_pose[2] = 0.50;
    pr.gravity = 9.81;
    pr.max_wsr = 100;
    wbc_ref_state st;
    wbc_ref_state_init(&st);
    st.method = method;
    int n_ok = 0, prev = 15;
    for (int k = 0; k < CYCLES; ++k) {
        const double t = k / 400.0, two_pi = 6.283185307179586;
        double pose[7] = {0}, nu[18] = {0}, qj[12], ref[54] = {0};
        /* a base that rolls, pitches and yaws: q = qz(yaw) qy(pitch) qx(roll), (x, y, z, w) */
        const double roll = 0.2 * sin(two_pi * 1.3 * t + 0.4), pitch = 0.15 * sin(two_pi * 0.9 * t + 1.1), yaw = 2.9 + 2.0 * t;
        const double cr = cos(roll / 2), sr = sin(roll / 2), cp = cos(pitch / 2), sp = sin(pitch / 2), cy = cos(yaw / 2), sy = sin(yaw / 2);
        pose[0] = 0.03 * sin(two_pi * t); pose[1] = 0.03 * sin(two_pi * t + 2.0); pose[2] = 0.585 + 0.03 * sin(two_pi * t + 4.0);
        pose[3] = sr * cp * cy - cr * sp * sy; pose[4] = cr * sp * cy + sr * cp * sy;
        pose[5] = cr * cp * sy - sr * sp * cy; pose[6] = cr * cp * cy + sr * sp * sy;
        nu[0] = 0.03 * two_pi * cos(two_pi * t); nu[1] = 0.03 * two_pi * cos(two_pi * t + 2.0); nu[2] = 0.03 * two_pi * cos(two_pi * t + 4.0);
        nu[3] = 0.3; nu[4] = -0.2; nu[5] = 2.0;
        for (int j = 0; j < 12; ++j) {
            qj[j] = Q0[j] + 0.2 * sin(two_pi * (0.5 + 0.2 * j) * t + j);
            nu[6 + j] = 0.2 * two_pi * (0.5 + 0.2 * j) * cos(two_pi * (0.5 + 0.2 * j) * t + j);
        }
        const int mask = MASKS[k / 3];
        ref[2] = 0.50;
        ref[5] = atan2(sin(yaw), cos(yaw));
        for (int l = 0; l < 4; ++l) {
            ref[18 + 3 * l] = cos(yaw) * FEET0[3 * l] - sin(yaw) * FEET0[3 * l + 1];
            ref[18 + 3 * l + 1] = sin(yaw) * FEET0[3 * l] + cos(yaw) * FEET0[3 * l + 1];
            ref[18 + 3 * l + 2] = ((mask >> l) & 1) ? 0.0 : 0.03;
        }
        /* latched for the first half, unlatched (derivatives differenced across the change) afterwards */
        const int switching = (k < CYCLES / 2) ? (mask != prev) : 0;
        prev = mask;
        const double* normals = k < 14 ? NORMALS[0] : k < 26 ? NORMALS[1] : NULL;
        double tau[12], grf[12], x[42];
        int iters = -1;
        wbc_ref_debug_t dbg;
        const int status = wbc_ref_step_normals(&WBC_ANYMAL_MODEL, &pr, &st, pose, nu, qj, ref, mask, switching, tau, grf, x, &iters, &dbg, normals);
        double s = 0.0;
        for (int j = 0; j < 12; ++j) s += fabs(tau[j]) + fabs(grf[j]);
        for (int j = 0; j < 42; ++j) s += fabs(x[j]);
        printf("method %d cycle %2d mask %2d switching %d status %d iters %2d |out|_1 %.6g\n", method, k, mask, switching, status, iters, s);
        if ((status != WBC_REF_OK && status != WBC_REF_INFEASIBLE) || !isfinite(s) || iters < 0) return 1;
        if (status != WBC_REF_OK && s != 0.0) return 1;
        n_ok += status == WBC_REF_OK;
    }
    return n_ok > 0 ? 0 : 1;
}

int main(void) {
    /* a cold batch of one through the batch entry point as well */
    double pose[7] = {0, 0, 0.585, 0, 0, 0, 1}, nu[18] = {0}, ref[54] = {0}, tau[12], grf[12], x[42];
    uint8_t con = 15, sw = 1;
    int32_t status = -1, iters = -1;
    ref[2] = 0.50;
    wbc_params pr;
    memset(&pr, 0, sizeof pr);
    pr.friction = 1.0; pr.loop_rate = 400.0; pr.max_torque = 80.0;
    pr.kp = 6000.0; pr.kp_z = 10000.0; pr.kd = 1800.0;
    pr.kp_swing = 250.0; pr.kd_swing = 20.0; pr.slack_weight = 1000.0;
    pr.initial_reference_pose[2] = 0.50;
    pr.gravity = 9.81;
    pr.max_wsr = 100;
    for (int method = 0; method < 2; ++method) {
        wbc_ref_run_batch_normals(&WBC_ANYMAL_MODEL, &pr, 1, pose, nu, Q0, ref, &con, &sw, tau, grf, x, &status, &iters, method, NORMALS[0]);
        printf("method %d cold batch of one: status %d iters %d\n", method, status, iters);
        if (status != WBC_REF_OK) return 1;
        if (run(method)) return 1;
    }
    printf("sanitize_normals: done\n");
    return 0;
}
