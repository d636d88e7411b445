/*
 * fdcn.h -- C ABI of the MI355X Crank-Nicolson finite-difference engine.
 *
 * TEST/PRODUCT BOUNDARY.  This header is the drop-in seam for the reference's
 * time-stepping hot path.  The reference (rwx-gigaba-sonwabo/Finite_Difference)
 * is pure Python and has no FFI; its seam is a pair of Python methods, which
 * the entry points below replace one-for-one:
 *
 *   fdcn_cn_batch  <- DiscreteBarrierFDMPricer._solve_grid
 *                       (discrete_barrier_fdm_pricer.py:442-547)
 *                     DiscreteBarrierCrankNicolsonLog._solve_grid
 *                       (discrete_barrier_fdm_pricer_cn.py:219-302)
 *                     KO projection _apply_KO_projection (…pricer.py:413-440,
 *                       …_cn.py:199-213) is fused in.
 *   fdcn_it_batch  <- AmericanFDMPricer._solve_segment
 *                       (fd_american_equity.py:559-726), Ikonen-Toivanen.
 *
 * The Python side (finite_difference_amd/capi.py) binds them with ctypes; the
 * binding a maintainer would add to the reference is in INTEGRATION.md.
 *
 * Conventions
 *   - A launch solves B independent scenarios ("solves") that share n_nodes,
 *     n_time and n_ranna.  Everything else is per scenario.
 *   - n_nodes counts ALL grid nodes including the two Dirichlet nodes:
 *     node 0 (S_min side), node n_nodes-1 (S_max side), interior 1..n_nodes-2.
 *     The production barrier engine's top-node drop (…pricer.py:449,543) is
 *     expressed by the caller passing n_nodes = N_s and v_init = payoff[0:N_s];
 *     the kernel has no quirk flag.  5 <= n_nodes <= 40962 (16 wavefronts
 *     x 64 lanes x 40 nodes + 2) is accepted: grids whose interior does not
 *     fill the lanes are padded with inactive lanes, 5-11-node grids run two
 *     nodes per lane; larger grids fail with FDCN_EINVAL.
 *   - Step m = 0..n_time-1 advances tau to tau_m = tau0 + (m+1)*dt and uses
 *     theta = 1 for m < n_ranna (Rannacher), 0.5 afterwards.
 *   - All arrays are C-contiguous, row-major, fp64 / int32.  The caller owns
 *     every buffer; nothing is retained after return.
 *   - Return 0 on success, a negative FDCN_E* code on failure; the message is
 *     available from fdcn_last_error() (thread-local).  Never aborts.
 */
#ifndef FDCN_H
#define FDCN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 8: fdcn_session_upload, fdcn_session_knockout and fdcn_session_march_ps (the
 * American knock-out chain: monitoring events between IT segments) were added
 * after 7; fdcn_session_knockin (the American knock-in chain) joined later as
 * an additive symbol, with the version left at 8.  So did the least-squares
 * Monte Carlo entry points (fdcn_mc_lsm_batch, fdcn_mc_lsm_batch_dev,
 * fdcn_mc_lsm_plan) and the Bermudan exercise event (fdcn_session_exercise,
 * fdcn_session_exercise_regions), and the quasi-Monte Carlo paths
 * (fdcn_mc_qmc_batch, fdcn_mc_qmc_batch_dev, fdcn_mc_qmc_plan; fdcn_qmc_normals
 * in fdcn_diag.h), and the least-squares Monte Carlo with cash dividends on
 * the path (fdcn_mc_lsm_div_batch, fdcn_mc_lsm_div_batch_dev), and the dual
 * upper bound of the least-squares Monte Carlo (fdcn_mc_lsm_dual_batch,
 * fdcn_mc_lsm_dual_batch_dev, fdcn_mc_lsm_dual_plan), and the dual and
 * table-policy bounds with cash dividends (fdcn_mc_lsm_dual_div_batch,
 * fdcn_mc_policy_div_batch, fdcn_mc_policy_dual_div_batch and their _dev
 * forms).
 * 7: the BGK barrier pricer's Monte Carlo entry points (fdcn_mc_bgk_batch,
 * fdcn_mc_bgk_batch_dev, fdcn_mc_bgk_plan) were added after 6.
 * 6: the Monte Carlo discrete-barrier entry points (fdcn_mc_barrier_batch,
 * fdcn_mc_barrier_batch_dev, fdcn_mc_plan; fdcn_mc_normals in fdcn_diag.h)
 * were added to the exported surface after 5.
 * 5: fdcn_session_host_buffer, the diagnostics of include/fdcn_diag.h for the
 * spot-space kernels (fdcn_vc_force_variant / _variant_name / _forms) and the
 * fdcn_vc workspace contract (+16 doubles per scenario) changed the exported
 * surface after 4 */
#define FDCN_ABI_VERSION 8

/* ---- per-scenario fp64 parameters: params[b*FDCN_NPARAM + k] ---------- */
enum fdcn_param {
  FDCN_P_DT = 0,  /* time step (years)                                       */
  FDCN_P_A,       /* operator coefficient of V_{j-1}: alpha - beta_adv       */
  FDCN_P_C,       /* operator coefficient of V_{j+1}: alpha + beta_adv       */
  FDCN_P_BC,      /* operator coefficient of V_j:     -2*alpha - r           */
  FDCN_P_TAU0,    /* tau at the start of this segment                        */
  FDCN_P_LO_C0,   /* lower Dirichlet value, see FDCN_I_LO_FORM               */
  FDCN_P_LO_E0,
  FDCN_P_LO_C1,
  FDCN_P_LO_E1,
  FDCN_P_HI_C0,   /* upper Dirichlet value, see FDCN_I_HI_FORM               */
  FDCN_P_HI_E0,
  FDCN_P_HI_C1,
  FDCN_P_HI_E1,
  FDCN_NPARAM
};

/* ---- per-scenario int32 parameters: iparams[b*FDCN_NIPARAM + k] ------- */
enum fdcn_iparam {
  FDCN_I_LO_FORM = 0, /* 0: c0*exp(e0*tau) + c1*exp(e1*tau)
                         1: ((c0*exp(e0*tau))*c1)*exp(e1*tau)  (…pricer.py:391) */
  FDCN_I_HI_FORM,
  FDCN_I_KO_LO,       /* monitor steps set V_j = rebate for j <= KO_LO (-1: none) */
  FDCN_I_KO_HI,       /* … and for j >= KO_HI (>= n_nodes: none)                 */
  FDCN_I_MON_START,   /* offset of this scenario's entries in mon_step/mon_rebate */
  FDCN_I_MON_COUNT,   /* number of entries: strictly increasing, values in 1..n_time
                         (the host entry points return FDCN_EINVAL otherwise; the
                         _dev kernels skip entries < 1 and entries not above the
                         previous one, as the oracle does) */
  FDCN_I_TAU_MODE,    /* tau after step m: 0: tau0 + (m+1)*dt (…pricer.py:519).
                         1: tau accumulated by repeated tau = tau + dt, as
                         fd_american_equity.py:664-724 does.  Both are honoured on
                         the device; any other value is FDCN_EINVAL (host entry
                         points) / treated as 0 (_dev). */
  FDCN_NIPARAM
};

/* error codes */
#define FDCN_OK 0
#define FDCN_EINVAL (-1)   /* bad argument / unsupported size                  */
#define FDCN_EHIP (-2)     /* HIP runtime error                                */
#define FDCN_ENODEV (-3)   /* no usable gfx950 device                          */
#define FDCN_ENOMEM (-4)   /* device allocation failed                         */

/* ---- host-pointer entry points (copy in, solve, copy out) ------------- */

/* European solve with knock-out projection on monitor steps.
 *   v_init     [B][n_nodes]  value vector at tau0 (payoff for a full solve)
 *   mon_step   [n_mon]       step numbers m+1 at which to project (per scenario
 *                            a sorted run addressed by MON_START/MON_COUNT)
 *   mon_rebate [n_mon]       value written into knocked-out nodes at that step
 *   v_out      [B][n_nodes]  value vector at tau0 + n_time*dt
 */
int fdcn_cn_batch(int32_t B, int32_t n_nodes, int32_t n_time, int32_t n_ranna,
                  const double* params, const int32_t* iparams,
                  const double* v_init,
                  int32_t n_mon, const int32_t* mon_step, const double* mon_rebate,
                  double* v_out);

/* American solve with Ikonen-Toivanen early exercise against payoff.
 *   payoff [B][n_nodes]  exercise value phi_j (only interior nodes are used);
 *   lambda starts at 0 in every call, as _solve_segment does (…equity.py:661).
 *   KO fields of iparams must be -1 / >= n_nodes and MON_COUNT 0.
 */
int fdcn_it_batch(int32_t B, int32_t n_nodes, int32_t n_time, int32_t n_ranna,
                  const double* params, const int32_t* iparams,
                  const double* v_init, const double* payoff,
                  double* v_out);

/* Threading: the host-pointer entry points are reentrant.  Each calling
 * thread gets its own non-blocking HIP stream on the current device
 * (fdcn_select_device / hipSetDevice), device buffers come stream-ordered
 * from the device's memory pool, and the call waits on its own stream only
 * (never a device-wide synchronisation).  The stream is created on a thread's
 * first call and kept for the thread's lifetime (it is not released when the
 * thread exits): issue calls from long-lived threads (a fixed pool), not from
 * a thread created per call. */

/* ---- device-pointer entry points (all pointers are device memory) ----- */
/* `stream` is a hipStream_t (NULL = default stream); the call is
 * asynchronous on that stream and performs no host sync.  Inputs and output
 * may alias (v_out == v_init) only if `v_init` is not needed afterwards.
 * `k_cap` bounds the boundary-layer correction table (see fdcn_sm_extent);
 * pass the value fdcn_sm_extent returns for the same params.  A scenario whose
 * extent exceeds k_cap gets NaN outputs (loud, never silently wrong).
 * `workspace` is device scratch of `workspace_bytes` bytes, at least
 * B * ws_bytes_per_scen as reported by fdcn_plan for the SAME B, n_nodes,
 * n_time, mode and k_cap (the kernel variant, and with it the workspace,
 * depends on B: small batches spread a scenario over more waves).  A smaller
 * (or negative) workspace_bytes is rejected with FDCN_EINVAL.  The Dirichlet
 * values of every step are evaluated there once per launch.  With NULL the
 * library allocates it stream-ordered (hipMallocAsync/hipFreeAsync on
 * `stream`, workspace_bytes ignored); pass a buffer to keep the call
 * allocation-free (e.g. for hipGraph capture). */
int fdcn_cn_batch_dev(int32_t B, int32_t n_nodes, int32_t n_time, int32_t n_ranna,
                      const double* params, const int32_t* iparams,
                      const double* v_init,
                      int32_t n_mon, const int32_t* mon_step, const double* mon_rebate,
                      double* v_out, int32_t k_cap, double* workspace,
                      int64_t workspace_bytes, void* stream);

int fdcn_it_batch_dev(int32_t B, int32_t n_nodes, int32_t n_time, int32_t n_ranna,
                      const double* params, const int32_t* iparams,
                      const double* v_init, const double* payoff,
                      double* v_out, int32_t k_cap, double* workspace,
                      int64_t workspace_bytes, void* stream);

/* ---- device-resident sessions (finite_difference_amd/csrc/fdcn_session.hip)
 * A session keeps solve outputs in HBM as numbered "slots" (one value vector
 * each) and chains marches, dividend jumps and the Greeks epilogue on the
 * device; only what the caller asks for comes back.  It replaces the host
 * round trips of
 *   _solve_grid -> _interp_price / _delta_gamma_from_grid / greeks
 *     (discrete_barrier_fdm_pricer.py:629-646, :883-904, :949-978;
 *      discrete_barrier_fdm_pricer_cn.py:429-466; fd_american_equity.py:855-1068)
 *   _solve_segment -> _apply_dividend_jump -> _solve_segment
 *     (fd_american_equity.py:479-553, :732-772, :825-843).
 * A session belongs to the thread's current device (fdcn_select_device) and is
 * not thread-safe; use one per thread.  Marches and jumps are asynchronous
 * (independent ones overlap on up to 4 session streams); greeks and fetch wait
 * for their inputs and return results.  Host arrays are staged through pinned
 * memory before a call returns.  After an error, destroy the session. */
typedef struct fdcn_session fdcn_session;
int fdcn_session_create(fdcn_session** out);
int fdcn_session_destroy(fdcn_session* s);
int fdcn_session_slots(const fdcn_session* s);  /* slots created so far */

/* `bytes` of pinned host memory owned by the session, valid until
 * fdcn_session_destroy (256-byte aligned).  A caller that builds a march's
 * payoff / v_init directly in it (the whole-file plans: 100-400 MB) spares
 * the staging copy: fdcn_session_march copies such an array to the device
 * from where it lies, asynchronously, so its contents must stay unchanged
 * until the session's next synchronising call (fdcn_session_greeks /
 * fdcn_session_fetch) or its destruction. */
int fdcn_session_host_buffer(fdcn_session* s, int64_t bytes, void** out);

/* One batched march (the fdcn_cn_batch / fdcn_it_batch plan; it != 0 for
 * Ikonen-Toivanen).  Initial vectors come from the host (v_init [B][n_nodes])
 * or from earlier slots (v_init_slots [B]); pass exactly one.  An IT march
 * may pass its payoff pointer as v_init (the array is copied once).  Host
 * arrays are staged through pinned memory before the call returns, except a
 * payoff / v_init inside an fdcn_session_host_buffer region (read later, by
 * the asynchronous copy).  The B outputs become new slots, numbers written
 * to out_slots [B]. */
int fdcn_session_march(fdcn_session* s, int32_t it, int32_t B, int32_t n_nodes, int32_t n_time,
                       int32_t n_ranna, const double* params, const int32_t* iparams,
                       const double* v_init, const int32_t* v_init_slots, const double* payoff,
                       int32_t n_mon, const int32_t* mon_step, const double* mon_rebate,
                       int32_t* out_slots);

/* fdcn_dividend_jump of B slots on the device: s_nodes [B][n_nodes] (host),
 * cash_div [B], strike_call [B] (< 0 for puts); results into new slots.
 * Bit-identical to fdcn_dividend_jump on the same inputs. */
int fdcn_session_dividend_jump(fdcn_session* s, int32_t B, int32_t n_nodes,
                               const int32_t* in_slots, const double* s_nodes,
                               const double* cash_div, const double* strike_call,
                               int32_t* out_slots);

/* Host vectors v [B][n_nodes] become B new slots (numbers into out_slots
 * [B]): the payoff of an American chain, uploaded once and then named by
 * fdcn_session_march_ps / fdcn_session_knockout.  Staged through pinned memory
 * before the call returns, or, for an array inside an
 * fdcn_session_host_buffer region, read in place by the asynchronous copy (as
 * fdcn_session_march does).  B >= 1, n_nodes >= 1. */
int fdcn_session_upload(fdcn_session* s, int32_t B, int32_t n_nodes, const double* v,
                        int32_t* out_slots);

/* Knock-out event of a discretely monitored American option, in place on
 * `slots` [B] (no new slot):
 *   V_j <- max(floor_j, rebate[b])   for j <= ko_lo[b] or j >= ko_hi[b]
 * with floor the vector in floor_slots[b] (the exercise value: the holder may
 * exercise an instant before the monitoring time); all other nodes keep their
 * value.  floor_slots == NULL: V_j <- rebate[b] (the plain projection).
 * Thresholds follow FDCN_I_KO_LO / FDCN_I_KO_HI (-1 / >= n_nodes: none on
 * that side); ko_lo[b] >= ko_hi[b] is allowed and knocks every node.
 * Bit-identical to np.where(knocked, np.maximum(floor, R), V).  The event is
 * ordered after every call the session queued before it (the march that
 * produced the slots, and any earlier reader of them); later consumers of the
 * slots wait for it.  B >= 1, n_nodes >= 1; a slot may appear once in
 * `slots`, and no floor slot may be one of `slots`. */
int fdcn_session_knockout(fdcn_session* s, int32_t B, int32_t n_nodes, const int32_t* slots,
                          const int32_t* ko_lo, const int32_t* ko_hi, const double* rebate,
                          const int32_t* floor_slots);

/* Knock-in event of a discretely monitored American option, in place on
 * `slots` [B] (no new slot):
 *   V_j <- src_j   for j <= ko_lo[b] or j >= ko_hi[b]
 * with src the vector in src_slots[b] (the vanilla American value the holder
 * owns once the barrier is seen breached: the coupled chain of the knock-in
 * march); all other nodes keep their value, and the source slots are only
 * read.  Thresholds follow FDCN_I_KO_LO / FDCN_I_KO_HI (-1 / >= n_nodes: none
 * on that side); ko_lo[b] >= ko_hi[b] copies every node.  Bit-identical to
 * np.where(knocked, src, V), NaNs included.  Ordered as
 * fdcn_session_knockout: after every call the session queued before it, and
 * later consumers of `slots` wait for it.  B >= 1, n_nodes >= 1; a slot may
 * appear once in `slots`, and no source slot may be one of `slots`.
 * Additive: the symbol joined the exported surface without a change of
 * FDCN_ABI_VERSION (still 8); a caller that needs it looks the symbol up. */
int fdcn_session_knockin(fdcn_session* s, int32_t B, int32_t n_nodes, const int32_t* slots,
                         const int32_t* src_slots, const int32_t* ko_lo, const int32_t* ko_hi);

/* Exercise event of a Bermudan option, in place on `slots` [B] (no new slot),
 * fused with the knock-out of a date that is also a monitoring date:
 *   V_j <- max(floor_j, rebate[b])   for j <= ko_lo[b] or j >= ko_hi[b]
 *   V_j <- max(V_j, floor_j)         on every other node
 * with floor the vector in floor_slots[b] (the exercise value, only read).
 * ko_lo, ko_hi and rebate all NULL: no barrier, no node is knocked; otherwise
 * all three are given and the thresholds follow fdcn_session_knockout.
 * Bit-identical to np.where(knocked, np.maximum(floor, R), np.maximum(V, floor))
 * for finite inputs (on a tie either operand is kept: the same bits except for
 * signed zeros); a NaN in either operand of a max gives NaN.
 * out_region_ids [B] receives the id of one exercise-region record per vector,
 * kept in session-owned device memory (ids are consecutive per session): lo,
 * hi and count of the nodes that are not knocked and had floor_j > V_j before
 * the event (a NaN compares false); without any, lo = n_nodes, hi = -1,
 * count = 0.  Read them with fdcn_session_exercise_regions.
 * Ordered as fdcn_session_knockout: after every call the session queued
 * before it, and later consumers of `slots` wait for it.  B >= 1, n_nodes >= 1
 * (the slots' length); a slot may appear once in `slots`, and no floor slot
 * may be one of `slots`.  Additive: the two symbols joined the exported
 * surface without a change of FDCN_ABI_VERSION (still 8). */
int fdcn_session_exercise(fdcn_session* s, int32_t B, int32_t n_nodes, const int32_t* slots,
                          const int32_t* floor_slots, const int32_t* ko_lo, const int32_t* ko_hi,
                          const double* rebate, int32_t* out_region_ids);

/* The exercise-region records `ids` [n] of this session into out [n][3] = lo,
 * hi, count.  Waits for the events that write them (synchronises).  n >= 0. */
int fdcn_session_exercise_regions(fdcn_session* s, int32_t n, const int32_t* ids, int32_t* out);

/* fdcn_session_march for an Ikonen-Toivanen march (it != 0 required) whose
 * payoff lies in earlier slots (payoff_slots [B], e.g. from
 * fdcn_session_upload) instead of a host array: a chain of segments names the
 * payoff it uploaded once rather than sending it with every march.  Slots
 * that are consecutive vectors of one block are read where they lie,
 * otherwise they are gathered on the device.  Same arithmetic, bit for bit,
 * as fdcn_session_march with the same payoff values.  B >= 1. */
int fdcn_session_march_ps(fdcn_session* s, int32_t it, int32_t B, int32_t n_nodes,
                          int32_t n_time, int32_t n_ranna, const double* params,
                          const int32_t* iparams, const double* v_init,
                          const int32_t* v_init_slots, const int32_t* payoff_slots,
                          int32_t n_mon, const int32_t* mon_step, const double* mon_rebate,
                          int32_t* out_slots);

/* Greeks epilogue: T trades, trade t of kind[t] reads readouts first[t] ..
 * first[t]+k-1 (k per kind below) and writes out[t][FDCN_GK_NOUT] =
 * price, delta, gamma, vega, theta, aux.  Readout r:
 *   rint[r][FDCN_GK_NRINT] = slot, interp case (0: between ilo and ilo+1,
 *                            1: V[0], 2: V[ilo]), ilo, idx, dg mode (0 none,
 *                            1 three-point at idx, 2 cubic through idx-1..idx+2)
 *   rdbl[r][FDCN_GK_NRDBL] = S_interp, s[ilo], s[ilo+1], S_dg, s[idx-1],
 *                            s[idx], s[idx+1], s[idx+2]
 * Node positions come from the host (bisection on its grids, as the pricers
 * do); the formulas keep the reference's operation order.  Kinds, params:
 *   FDCN_GK_BARRIER  2 readouts (base: interp + 3-point; sigma-bumped: interp)
 *                    P = sigma, spot, carry, div_yield, r, dv   (…pricer.py:883-904)
 *   FDCN_GK_CNLOG    3 readouts (base, sigma+dv, sigma-dv)
 *                    P = sigma, S0, b, r, dv                    (…_cn.py:429-466)
 *   FDCN_GK_AMERICAN 7 readouts (N and 2N: interp + cubic; sigma +h, -h, +2h,
 *                    -2h at N; N_t = 2 num_space_nodes) P = sigma, spot, carry, r, h;
 *                    aux = price_log2's Richardson       (fd_american_equity.py:925-1068)
 *   FDCN_GK_READOUT  1 readout: price, delta, gamma of that vector */
#define FDCN_GK_BARRIER 0
#define FDCN_GK_CNLOG 1
#define FDCN_GK_AMERICAN 2
#define FDCN_GK_READOUT 3
#define FDCN_GK_NPARAM 8
#define FDCN_GK_NRINT 5
#define FDCN_GK_NRDBL 8
#define FDCN_GK_NOUT 6
int fdcn_session_greeks(fdcn_session* s, int32_t T, const int32_t* kind, const int32_t* first,
                        const double* tparams, int32_t R, const int32_t* rint,
                        const double* rdbl, double* out);

/* Copy n slots (each n_nodes long) back to out [n][n_nodes]. */
int fdcn_session_fetch(fdcn_session* s, int32_t n, const int32_t* slots, int32_t n_nodes,
                       double* out);

/* ---- launch planning / introspection ---------------------------------- */
/* Writes the kernel geometry a launch of B scenarios uses: waves per
 * scenario, nodes per lane, scenarios per workgroup (2: the paired flavour,
 * two scenarios per wavefront, used for large batches of <= 256-node grids),
 * LDS bytes per workgroup, and the device workspace the _dev entry points
 * need per scenario.  Batches too small to fill the chip spread each scenario
 * over more waves, so the plan depends on B; call it with the B you launch.
 * Any output pointer may be NULL.  Returns FDCN_EINVAL if the size is
 * unsupported. */
int fdcn_plan(int32_t B, int32_t n_nodes, int32_t n_time, int32_t it_mode, int32_t k_cap,
              int32_t* waves, int32_t* npt, int32_t* scen_per_block, int32_t* lds_bytes,
              int64_t* ws_bytes_per_scen);

/* Extent (nodes) of the Sherman-Morrison boundary-layer correction needed by
 * the scenarios in `params` (host memory): the largest k such that the
 * correction at interior node k is above 1e-18 of its value at node 0, over
 * both theta values used by the launch.  Returns a value in [1, n_nodes-2],
 * or a negative FDCN_E* code. */
int fdcn_sm_extent(int32_t B, int32_t n_nodes, int32_t n_time, int32_t n_ranna,
                   const double* params);

/* ---- spot-space CN with per-row coefficients ---------------------------
 * fdcn_vc_batch <- DiscreteBarrierFDMPricer2._solve_pde_backward
 *                    (discrete_barrier_fdm_pricer_2.py:336-428, FIS barrier
 *                    rows and BGK window) and
 *                  DiscreteBarrierFDMPricerAnalytic._cn_stepper
 *                    (discrete_barrier_analytic_pricer.py:384-432).
 * The matrices are tridiagonal with a different row at every node (uniform S
 * grid, sigma^2 S_i^2 terms, the non-symmetric rows at the barrier), constant
 * in time within a phase: phase 0 for steps m < n_ranna (Rannacher), phase 1
 * after.  Step m: rhs_i = a_i V_{i-1} + b_i V_i + c_i V_{i+1} for interior
 * rows, rhs_0 = bnd[m][0], rhs_{n-1} = bnd[m][1]; solve
 * sub_i x_{i-1} + main_i x_i + sup_i x_{i+1} = rhs_i (sub_0 = sup_{n-1} = 0);
 * V = x; then the knock-out projection of the CN ABI (iparams KO_LO / KO_HI,
 * MON_START / MON_COUNT; LO/HI_FORM and TAU_MODE unused, pass 0).
 *   diag [B][2][FDCN_VC_NDIAG][n_nodes]  sub, main, sup, a, b, c per phase
 *   bnd  [B][n_time][2]                  Dirichlet values of rows 0 / n-1
 * The LU factors of each phase are computed once per launch; the march
 * keeps the rows' factored coefficients and V in registers. */
#define FDCN_VC_NDIAG 6
int fdcn_vc_batch(int32_t B, int32_t n_nodes, int32_t n_time, int32_t n_ranna,
                  const double* diag, const double* bnd, const double* v_init,
                  const int32_t* iparams, int32_t n_mon, const int32_t* mon_step,
                  const double* mon_rebate, double* v_out);
int fdcn_vc_batch_dev(int32_t B, int32_t n_nodes, int32_t n_time, int32_t n_ranna,
                      const double* diag, const double* bnd, const double* v_init,
                      const int32_t* iparams, int32_t n_mon, const int32_t* mon_step,
                      const double* mon_rebate, double* v_out, double* workspace,
                      int64_t workspace_bytes, void* stream);
/* geometry of a fdcn_vc launch of B scenarios (depends on B): waves per
 * scenario, nodes per lane, device workspace per scenario (bytes) */
int fdcn_vc_plan(int32_t B, int32_t n_nodes, int32_t* waves, int32_t* npt,
                 int64_t* ws_bytes_per_scen);

/* ---- batched closed-form barrier engines (one thread per contract) ------ */
/* Reiner-Rubinstein single continuous barrier with cash rebate and barrier
 * status; replaces BarrierEngine(s,b,r,t,x,sigma,h,optionflag,directionflag,
 * in_out_flag,k,barrier_status,rebate_timing_in,rebate_timing_out).price() /
 * .vanilla() (barrier_engine.py:38-44, 189) for B contracts at once.
 *   params[B][FDCN_RR_NPARAM] = s, b, r, t, x (strike), sigma, h (barrier), k (rebate)
 *   flags [B][FDCN_RR_NFLAG]  = option (0 call, 1 put), direction (0 up, 1 down),
 *                               in/out (0 in, 1 out), status (0 not crossed, 1 crossed),
 *                               rebate timing bits (1: knock-in rebate paid at hit,
 *                               2: knock-out rebate paid at expiry; defaults 0)
 *   price[B], vanilla[B] (the A factor).  */
#define FDCN_RR_NPARAM 8
#define FDCN_RR_NFLAG 5
int fdcn_rr_barrier_batch(int32_t B, const double* params, const int32_t* flags,
                          double* price, double* vanilla);
int fdcn_rr_barrier_batch_dev(int32_t B, const double* params, const int32_t* flags,
                              double* price, double* vanilla, void* stream);

/* Double knock-out / knock-in (Ikeda-Kunitomo / Douady series, n = -m..m);
 * replaces DoubleBarrier(S,X,L,U,sigma,callflag,inflag,m).price(b,r,T)
 * (double _barrier.py:33-134).
 *   params[B][FDCN_DB_NPARAM] = S, X, L, U, sigma, b, r, T
 *   flags [B][FDCN_DB_NFLAG]  = option (0 call, 1 put), in/out (0 in, 1 out),
 *                               corrected put (0: the reference's alpha = 1, :95)
 *   price[B]. */
#define FDCN_DB_NPARAM 8
#define FDCN_DB_NFLAG 3
int fdcn_double_barrier_batch(int32_t B, int32_t m, const double* params,
                              const int32_t* flags, double* price);
int fdcn_double_barrier_batch_dev(int32_t B, int32_t m, const double* params,
                                  const int32_t* flags, double* price, void* stream);

/* ---- Monte Carlo discrete-barrier pricer (finite_difference_amd/csrc/fdcn_mc.hip)
 * fdcn_mc_barrier_batch <- price_discrete_barrier_mc's path loop and estimator
 *                          (mc_discrete_barrier_option.py:314-410).
 * One launch prices B contracts that share n_steps, n_obs and `antithetic`;
 * the host computes every curve quantity (event grid, carry per interval,
 * discount factors, the barrier band).
 *   params[B][FDCN_MC_NPARAM]        see enum fdcn_mc_param
 *   flags [B][FDCN_MC_NFLAG]         see enum fdcn_mc_flag
 *   step  [B][n_steps][FDCN_MC_NSTEP] see enum fdcn_mc_step
 * Path, per step i (the reference's order):  s *= exp(drift + diff * z_i);
 * the cash dividend s = max(s - D, floor) before the monitor check if
 * DIV_FIRST, after it otherwise; on a monitor step the breach test
 * s <= threshold (down kinds) / s >= threshold (up kinds).  At the end the
 * vanilla payoff max(+-(s - strike), 0) * df_T: paid to untouched paths
 * (knock-out), to touched paths (knock-in), to all (kind 0); a knocked-out
 * path pays rebate * df_T, or rebate * DF_END of its first hit step with
 * REBATE_AT_HIT.  An observation is f(Z), or 0.5 * (f(Z) + f(-Z)) with
 * antithetic != 0; n_obs counts observations.
 *
 * Normals.  z != NULL: z [n_obs][n_steps], shared by all B contracts (the
 * reference shares one stream per call); observation i reads row i.
 * z == NULL: generated with Philox4x32-10.  This mapping is a contract:
 *   counter = (o & 0xffffffff, o >> 32, j, stream id),  o = obs_first + i,
 *   key     = (seed & 0xffffffff, seed >> 32),
 *   x0..x3  = Philox4x32-10(counter, key)   (Random123: multipliers D2511F53,
 *             CD9E8D57; key increments 9E3779B9, BB67AE85),
 *   u1 = ((x0 >> 5) * 2^26 + (x1 >> 6) + 0.5) * 2^-53,  u2 likewise from x2, x3
 *        (evaluated in fp64 in that order),
 *   z[2j]   = sqrt(-2 ln u1) * cospi(2 u2),
 *   z[2j+1] = sqrt(-2 ln u1) * sinpi(2 u2)   (dropped when 2j+1 == n_steps).
 * Disjoint [obs_first, obs_first + n_obs) ranges of one (seed, stream id)
 * continue one stream: ranks shard the paths of a contract, or a run resumes,
 * and sum p / sum p^2 of the parts add up.
 *
 * Reduction.  Deterministic, no floating-point atomics: a workgroup owns a
 * fixed chunk of observations (fdcn_mc_plan: a function of n_obs only), each
 * thread adds its observations in index order, the workgroup reduces in a
 * fixed tree, and a second kernel adds the per-workgroup partials in order.
 * A contract's result depends on neither B nor its position in the batch.
 *   stats [B][FDCN_MC_NSTAT] = price = sum p / n, stderr =
 *                              sqrt(max(0, sum p^2 / n - price^2) / n),
 *                              sum p, sum p^2
 *   payoff_out [B][n_obs]      the observations (NULL: not written)
 * Validation (before any device call; FDCN_EINVAL): B, n_steps, n_obs < 1;
 * antithetic or a flag out of range; NULL params / flags / step / stats; and,
 * host entry only, spot or strike <= 0, threshold <= 0 where KIND != 0. */
#define FDCN_MC_NPARAM 6
enum fdcn_mc_param {
  FDCN_MC_P_SPOT = 0,
  FDCN_MC_P_STRIKE,
  FDCN_MC_P_DF_T,      /* discount factor to maturity                          */
  FDCN_MC_P_THRESHOLD, /* level + band (down kinds) / level - band (up kinds)  */
  FDCN_MC_P_REBATE,    /* cash amount paid to a knocked-out path               */
  FDCN_MC_P_FLOOR      /* spot floor after a cash dividend                     */
};
#define FDCN_MC_NFLAG 5
enum fdcn_mc_flag {
  FDCN_MC_F_PUT = 0,       /* 0 call, 1 put                                      */
  FDCN_MC_F_KIND,          /* 0 none, 1 down-out, 2 up-out, 3 down-in, 4 up-in   */
  FDCN_MC_F_REBATE_AT_HIT, /* 1: the rebate is discounted from its hit date      */
  FDCN_MC_F_DIV_FIRST,     /* 1: dividend_before_monitor                         */
  FDCN_MC_F_STREAM         /* Philox stream id (>= 0), counter word 3            */
};
#define FDCN_MC_NSTEP 5
enum fdcn_mc_step {
  FDCN_MC_S_DRIFT = 0, /* (carry - sigma^2 / 2) * tau                           */
  FDCN_MC_S_DIFF,      /* sigma * sqrt(tau)                                     */
  FDCN_MC_S_DIV,       /* cash dividend at the step's end date (0: none)        */
  FDCN_MC_S_MONITOR,   /* 1.0 if the end date is monitored, else 0.0            */
  FDCN_MC_S_DF_END     /* discount factor at the end date (rebate at hit)       */
};
#define FDCN_MC_NSTAT 4
/* Host pointers; copies in and out on the calling thread's stream (see
 * "Threading" above) and waits for it. */
int fdcn_mc_barrier_batch(int32_t B, int32_t n_steps, int64_t n_obs, int32_t antithetic,
                          const double* params, const int32_t* flags, const double* step,
                          const double* z, uint64_t seed, int64_t obs_first, double* stats,
                          double* payoff_out);
/* Device pointers, asynchronous on `stream`, no host sync.  `workspace` is
 * device scratch of at least B * ws_bytes_per_contract (fdcn_mc_plan) bytes
 * -- a smaller workspace_bytes is FDCN_EINVAL -- or NULL: allocated
 * stream-ordered for the call.  The flags are device memory, so their range
 * is not checked here: the kernel treats a KIND outside 0..4 as 0. */
int fdcn_mc_barrier_batch_dev(int32_t B, int32_t n_steps, int64_t n_obs, int32_t antithetic,
                              const double* params, const int32_t* flags, const double* step,
                              const double* z, uint64_t seed, int64_t obs_first, double* stats,
                              double* payoff_out, double* workspace, int64_t workspace_bytes,
                              void* stream);
/* Geometry of a launch of n_obs observations per contract: workgroups per
 * contract, observations per workgroup, workspace bytes per contract.  Any
 * output pointer may be NULL.  Host only. */
int fdcn_mc_plan(int64_t n_obs, int32_t* blocks_per_contract, int32_t* obs_per_block,
                 int64_t* ws_bytes_per_contract);

/* ---- Quasi-Monte Carlo paths of the same pricer (csrc/fdcn_mc_qmc.hip) ------
 * fdcn_mc_qmc_batch prices the contracts of fdcn_mc_barrier_batch (the same
 * params / flags / step arrays and enums, the same path functional) on R
 * randomised replicates of n_obs Sobol points each, the normals laid onto the
 * path through a caller-supplied construction table.  An additive symbol:
 * FDCN_ABI_VERSION is still 8.  Every number below is a contract, evaluated in
 * fp64 with each operation rounded separately.
 *
 * Observation o = obs_first + i (o < 2^32), replicate rho = rep_first + k.
 * Sobol word of dimension j = 0 .. n_steps - 1:
 *   g   = o ^ (o >> 1)                                   (Gray-code order)
 *   w_j = XOR over the set bits k of g of dirnum[j][k]
 *   dirnum [n_steps][32] uint32, left-aligned (bit 31 is 1/2), supplied by the
 *   caller; the library embeds no table.  With a table of the usual
 *   Joe-Kuo kind, point o is the o-th unscrambled draw of the sequence.
 * Digital shift (scramble = 1):
 *   w_j ^= x0 of Philox4x32-10(counter = (j, rho, 0, stream id),
 *                              key = (seed & 0xffffffff, seed >> 32)),
 *   the block function of fdcn_mc_barrier_batch above, stream id =
 *   flags[FDCN_MC_F_STREAM].  scramble = 0 applies no shift; it requires R = 1
 *   and reports stderr 0.
 * Uniform:  u = ((double)w_j + 0.5) * 2^-32, never 0 or 1; 1 - u is exact.
 * Normal:   y_j = Phi^-1(u) by Wichura's algorithm AS241, routine PPND16, with
 *   the branches, constants and Horner order of CPython's
 *   statistics._normal_dist_inv_cdf: q = u - 0.5; for |q| <= 0.425 a rational
 *   function in 0.180625 - q^2 times q (no transcendental: bit for bit the
 *   same in any IEEE arithmetic); otherwise r = sqrt(-log(min(u, 1 - u))),
 *   r <= 5: rational in r - 1.6, else rational in r - 5; negated for q < 0.
 * Path construction:
 *   bridge_idx [n_steps][3] int32 = target, left, right -- shared by the
 *               launch, always host memory (it reaches the kernel by value);
 *   bridge_w   [B][n_steps][3]    = wl, wr, sd -- per contract;
 *   W[0] = 0;  for j = 0 .. n_steps - 1:
 *     W[target_j] = (wl_j * W[left_j] + wr_j * W[right_j]) + sd_j * y_j;
 *   step m = 1 .. n_steps:  s *= exp(DRIFT_m + (W[m] - W[m-1])), then the
 *   dividend, monitor test and hit discount factor of fdcn_mc_barrier_batch.
 *   The DIFF column is not read.  With antithetic != 0 the mirrored path walks
 *   -W and the observation is 0.5 * (f(W) + f(-W)).
 * Reduction.  One workgroup owns one (contract, replicate, chunk of
 * observations); the chunk (fdcn_mc_qmc_plan) is a function of n_steps and
 * n_obs only.  Each thread adds its observations in index order, the workgroup
 * reduces in a fixed tree, a second kernel adds the partials of a replicate in
 * block order and combines the replicates in replicate order.  No
 * floating-point atomics: a contract's numbers depend on neither B nor its
 * position in the batch.  With m_rho = (sum p of replicate rho) / n_obs:
 *   stats [B][FDCN_MC_NSTAT] = price = (sum m_rho) / R,
 *                              stderr = sqrt(sum (m_rho - price)^2 / (R-1) / R)
 *                                       (0 for R = 1),
 *                              sum m_rho, sum m_rho^2
 *   rep_out [B][R][2]          sum p, sum p^2 of each replicate (NULL: not written)
 *   payoff_out [B][R][n_obs]   the observations (NULL: not written)
 * Sharding.  Disjoint rep_first ranges are independent replicates; disjoint
 * obs_first ranges of one replicate continue one point set.  The per-replicate
 * sums of the parts add.
 * Validation (before any device call; FDCN_EINVAL): B, n_obs or R < 1; n_steps
 * outside 1 .. FDCN_QMC_MAX_STEPS; antithetic or scramble not 0 / 1;
 * scramble == 0 with R != 1; obs_first < 0, obs_first + n_obs > 2^32,
 * rep_first < 0; a NULL params / flags / step / dirnum / bridge_idx /
 * bridge_w / stats; a workspace that is too small; a bridge_idx row that
 * breaks one of: target in 1 .. n_steps, each target once; left < target and
 * already defined (0 or an earlier target); right > target and already
 * defined, or right == left (an extension past the known range: row 0 of a
 * bridge, every row of an incremental construction).  Host entry only: the
 * per-contract checks of fdcn_mc_barrier_batch and a non-finite bridge_w. */
#define FDCN_QMC_MAX_STEPS 64
/* Host pointers; copies in and out on the calling thread's stream and waits. */
int fdcn_mc_qmc_batch(int32_t B, int32_t n_steps, int64_t n_obs, int32_t R, int32_t antithetic,
                      int32_t scramble, const double* params, const int32_t* flags,
                      const double* step, const uint32_t* dirnum, const int32_t* bridge_idx,
                      const double* bridge_w, uint64_t seed, int64_t obs_first, int32_t rep_first,
                      double* stats, double* rep_out, double* payoff_out);
/* Device pointers except bridge_idx (host), asynchronous on `stream`, no host
 * sync.  `workspace`: device scratch of at least B * ws_bytes_per_contract
 * (fdcn_mc_qmc_plan) bytes, or NULL: allocated stream-ordered for the call. */
int fdcn_mc_qmc_batch_dev(int32_t B, int32_t n_steps, int64_t n_obs, int32_t R, int32_t antithetic,
                          int32_t scramble, const double* params, const int32_t* flags,
                          const double* step, const uint32_t* dirnum, const int32_t* bridge_idx,
                          const double* bridge_w, uint64_t seed, int64_t obs_first,
                          int32_t rep_first, double* stats, double* rep_out, double* payoff_out,
                          double* workspace, int64_t workspace_bytes, void* stream);
/* Geometry of a launch: workgroups per (contract, replicate), observations per
 * workgroup (256 threads x 16 up to 30 steps, 64 x 16 above), workspace bytes
 * per contract.  Any output pointer may be NULL.  Host only. */
int fdcn_mc_qmc_plan(int32_t n_steps, int64_t n_obs, int32_t R, int32_t* blocks_per_replicate,
                     int32_t* obs_per_block, int64_t* ws_bytes_per_contract);

/* ---- Monte Carlo paths of the BGK barrier pricer (csrc/fdcn_mc_bgk.hip) ----
 * fdcn_mc_bgk_batch <- DiscreteBarrierBGKPricer._mc_out_price's path functional
 *                      (discrete_barrier_bgk.py:770-878).
 * One launch prices B trades x G scenarios (1 <= G <= FDCN_BGK_MAX_G) that
 * share n_steps, n_obs, `antithetic` and G.  The G scenarios of a trade (the
 * bumped re-pricings of its Greeks) share the trade's flags and its normals:
 * an observation's normals are drawn once and every scenario, and both signs,
 * walk them.
 *   params[B][G][FDCN_BGK_NPARAM]          see enum fdcn_bgk_param
 *   flags [B][FDCN_BGK_NFLAG]              see enum fdcn_bgk_flag
 *   step  [B][G][n_steps][FDCN_BGK_NSTEP]  see enum fdcn_bgk_step
 * Path (every operation rounded separately, in this order).  Per step k:
 * c += drift_k + diff_k * z_k (the mirrored path: drift_k - diff_k * z_k).
 * On a monitored step S = exp(log_spot + c) and
 *   event = max(max(0, up(S)), down(S)) over the active sides, where for a
 *   barrier epsilon e > 0   up = 0 if S < Hu - e, 1 if S > Hu + e, else
 *   0.5 + (S - Hu) / (2 e);  down = 1 if S < Hd - e, 0 if S > Hd + e, else
 *   0.5 + (Hd - S) / (2 e);  and for e = 0  up = [S >= Hu], down = [S <= Hd];
 *   rebate mode 2, e > 0:  newly = max(0, event - [rebate_pv > 0]),
 *                          rebate_pv += (newly * R) * DF_END_k;
 *   rebate mode 2, e = 0:  the first hit sets rebate_pv = R * DF_END_k;
 *   breached += event.
 * At the end S_T = exp(log_spot + c), alive = clip(1 - breached, 0, 1),
 * d = S_T - K (call) or K - S_T (put), intrinsic = max(d, 0) for a payoff
 * epsilon p = 0, else 0 if d < -p, d if d > p, else
 * (0.5 d^2 + p d + 0.5 p^2) / (2 p);  x = alive * intrinsic, plus
 * R * (1 - alive) in rebate mode 1.
 * Paths: n_sim = n_obs * (1 + antithetic); path i is +z of observation i,
 * path n_obs + i is -z.  Normals: z [n_obs][n_steps] shared by the launch, or
 * NULL: the Philox mapping of fdcn_mc_barrier_batch above (counter = (o low,
 * o high, pair, stream id), o = obs_first + i; key = seed), so disjoint
 * obs_first ranges continue one stream and the sums of the parts add.
 *   stats [B][G][FDCN_BGK_NSTAT] = raw sums over the n_sim paths: sum x,
 *                                  sum x^2, sum rebate_pv, sum (1 - alive)
 *   payoff_out [B][G][2][n_sim]    x, then rebate_pv (NULL: not written)
 * The caller composes price and standard error (the pricer: DF_T * mean x +
 * mean rebate_pv; sqrt((sum x^2 - (sum x)^2 / n) / (n - 1)) * DF_T / sqrt n).
 * Reduction: as fdcn_mc_barrier_batch -- no floating-point atomics, a fixed
 * chunk (fdcn_mc_bgk_plan), fixed tree, partials added in block order.  A
 * scenario's sums are bit-identical whatever G, its slot, B, or the trade's
 * position in the batch.
 * Validation (before any device call; FDCN_EINVAL): B, n_steps, n_obs < 1; G
 * outside 1..8; antithetic out of range; NULL params / flags / step / stats;
 * and, host entry only: put, sides (0..3), rebate mode (0..2) or stream id out
 * of range; a non-finite log-spot; strike <= 0; a negative epsilon; a level
 * <= 0 on an active side. */
#define FDCN_BGK_MAX_G 8
#define FDCN_BGK_NPARAM 7
enum fdcn_bgk_param {
  FDCN_BGK_P_LOG_SPOT = 0, /* ln(spot), computed by the caller                  */
  FDCN_BGK_P_STRIKE,
  FDCN_BGK_P_UPPER,        /* upper level Hu (read if sides bit 0)               */
  FDCN_BGK_P_LOWER,        /* lower level Hd (read if sides bit 1)               */
  FDCN_BGK_P_EPS_BARRIER,  /* half-width of the smoothed barrier test; 0: exact  */
  FDCN_BGK_P_EPS_PAYOFF,   /* half-width of the smoothed payoff; 0: exact        */
  FDCN_BGK_P_REBATE        /* cash rebate R                                      */
};
#define FDCN_BGK_NFLAG 4
enum fdcn_bgk_flag {
  FDCN_BGK_F_PUT = 0,      /* 0 call, 1 put                                      */
  FDCN_BGK_F_SIDES,        /* bit 0 upper active, bit 1 lower active, 0 vanilla  */
  FDCN_BGK_F_REBATE_MODE,  /* 0 none, 1 at expiry, 2 at hit                      */
  FDCN_BGK_F_STREAM        /* Philox stream id (>= 0), counter word 3            */
};
#define FDCN_BGK_NSTEP 4
enum fdcn_bgk_step {
  FDCN_BGK_S_DRIFT = 0, /* (mu - sigma^2 / 2) * dt                               */
  FDCN_BGK_S_DIFF,      /* sigma * sqrt(dt)                                      */
  FDCN_BGK_S_MONITOR,   /* 1.0 if the step's end is monitored, else 0.0; the same
                           for the G scenarios of a trade                        */
  FDCN_BGK_S_DF_END     /* discount factor at the step's end (rebate at hit)     */
};
#define FDCN_BGK_NSTAT 4
/* Host pointers; copies in and out on the calling thread's stream and waits. */
int fdcn_mc_bgk_batch(int32_t B, int32_t G, int32_t n_steps, int64_t n_obs, int32_t antithetic,
                      const double* params, const int32_t* flags, const double* step,
                      const double* z, uint64_t seed, int64_t obs_first, double* stats,
                      double* payoff_out);
/* Device pointers, asynchronous on `stream`, no host sync.  `workspace` is
 * device scratch of at least B * ws_bytes_per_trade (fdcn_mc_bgk_plan) bytes
 * -- a smaller workspace_bytes is FDCN_EINVAL -- or NULL: allocated
 * stream-ordered for the call.  The flags are device memory, so their range is
 * not checked here: the kernel masks sides to two bits and treats a rebate
 * mode outside 0..2 as 0. */
int fdcn_mc_bgk_batch_dev(int32_t B, int32_t G, int32_t n_steps, int64_t n_obs,
                          int32_t antithetic, const double* params, const int32_t* flags,
                          const double* step, const double* z, uint64_t seed, int64_t obs_first,
                          double* stats, double* payoff_out, double* workspace,
                          int64_t workspace_bytes, void* stream);
/* Geometry of a launch of n_obs observations per trade at group size G:
 * workgroups per trade, observations per workgroup (a constant), workspace
 * bytes per trade.  Any output pointer may be NULL.  Host only. */
int fdcn_mc_bgk_plan(int64_t n_obs, int32_t G, int32_t* blocks_per_trade, int32_t* obs_per_block,
                     int64_t* ws_bytes_per_trade);

/* ---- Least-squares Monte Carlo for American / Bermudan options with discrete
 * barriers (csrc/fdcn_mc_lsm.hip): the statistical cross-check of the
 * early-exercise FD pricers (Longstaff-Schwartz, out-of-sample estimator).
 * One launch prices B contracts that share n_steps, G and `antithetic`.
 *   params[B][FDCN_LSM_NPARAM]          see enum fdcn_lsm_param
 *   flags [B][FDCN_LSM_NFLAG]           see enum fdcn_lsm_flag
 *   step  [B][n_steps][FDCN_LSM_NSTEP]  see enum fdcn_lsm_step; row m - 1 is
 *                                       step m = 1 .. n_steps, ending at t_m
 * A contract is G sub-runs; one workgroup owns one sub-run: FDCN_LSM_SUBRUN
 * paths, a complete LSM of its own (fit, then price on fresh paths).  Path p
 * of a sub-run is slot k = p / 256 of thread p % 256.  Without antithetic
 * path p is observation p; with it a sub-run has FDCN_LSM_SUBRUN / 2
 * observations, path p is observation (k / 2) * 256 + p % 256 with +z for k
 * even and -z for k odd.  Every operation below is rounded separately.
 *
 * A, fit set forward: x = ln(spot); x += DRIFT_m + DIFF_m * z_m for m = 1 ..
 * n_steps; s = exp(x); h = the first MONITOR step with s <= lower (kinds with
 * a lower level) or s >= upper (kinds with an upper level), n_steps + 1 if
 * none.
 * B, fit set backward, m = n_steps .. 1, x and the payoff phi = max(+-(exp(x)
 * - strike), 0) at t_m, cf the realised cashflow discounted to t_m:
 *   m = n_steps   knock-out: cf = max(phi, REBATE_m) if h == m, phi if h > m;
 *                 knock-in:  cf = phi if h <= m, else REBATE_m;  none: phi.
 *   m < n_steps   x -= DRIFT_{m+1} + DIFF_{m+1} * z_{m+1}, cf *= DF_STEP_{m+1};
 *                 a knock-out path with h == m: cf = max(phi, REBATE_m) (the
 *                 exercise floor of the FD knock-out); then, on an EXERCISE
 *                 step, the eligible paths (knock-out: m < h, knock-in: m >= h,
 *                 none: all) with phi > 0 enter a cubic least-squares fit of
 *                 cf on u = (x - CENTRE_m) * ISCALE_m: the twelve sums
 *                 sum u^0 .. u^6, sum u^k cf (k = 0 .. 3) and the count, each
 *                 thread in slot order, then a fixed tree; an unpivoted 4 x 4
 *                 Cholesky in a fixed order on every lane.  The fit is invalid
 *                 with fewer than FDCN_LSM_MIN_FIT paths or a pivot d_j <=
 *                 1e-12 * a_jj: no voluntary exercise at that step.  Otherwise
 *                 fit(u) = c0 + u (c1 + u (c2 + u c3)) and a path of the fit
 *                 exercises where phi > fit(u), strictly: cf = phi.
 *   The in-sample value of a path is cf * DF_STEP_1.
 * C, price set forward (independent normals): the path stops at the first
 * step where the event rule (knock-out breach: max(phi, REBATE_m); maturity)
 * or the fitted rule (EXERCISE step, valid fit, eligible, phi > 0, phi >
 * fit(u)) says so; its value is the cashflow times DF_END_m.  A knock-in
 * breach at step m makes the path eligible from m on, m included.
 *
 * Normals: the Philox mapping of fdcn_mc_barrier_batch with counter word 3 =
 * 2 * stream id (fit set) or 2 * stream id + 1 (price set), stream id < 2^30:
 *   counter = (o low, o high, pair, stream word), key = seed,
 *   o = obs_first + g * (observations per sub-run) + i for observation i of
 *   sub-run g.  obs_first must be a multiple of the observations per sub-run:
 *   disjoint sub-run ranges of one (seed, stream id) are shards of one run,
 *   and their (G, sum, sum of squares) of the sub-run means merge.
 * Reduction: no floating-point atomics; sums per thread in slot order, a fixed
 * tree, one partial per sub-run, added in sub-run order by a second kernel.  A
 * contract's numbers depend on neither B nor its position in the batch.
 *   stats [B][FDCN_LSM_NSTAT]           see enum fdcn_lsm_stat
 *   values_out [B][G * FDCN_LSM_SUBRUN] price-set value per path (NULL: none)
 *   coef_out [B][G][n_steps][FDCN_LSM_NCOEF]  c0 .. c3 and 1.0 / 0.0 for a
 *                                       valid fit, zeros at steps without a
 *                                       fit (NULL: none)
 * Validation (before any device call; FDCN_EINVAL): B, G < 1; n_steps outside
 * 1 .. FDCN_LSM_MAX_STEPS; B * G beyond a grid; antithetic out of range;
 * obs_first negative or misaligned; NULL params / flags / step / stats; and,
 * host entry only: put, kind (0 .. 6) or stream id (0 .. 2^30 - 1) out of
 * range; spot or strike <= 0; a level <= 0 where the kind reads it, lower >=
 * upper for a double barrier; a step with DIFF <= 0 (sigma must be positive),
 * ISCALE <= 0 or a non-finite entry. */
#define FDCN_LSM_MAX_STEPS 512
#define FDCN_LSM_SUBRUN 4096
#define FDCN_LSM_MIN_FIT 64
#define FDCN_LSM_NCOEF 5
#define FDCN_LSM_NPARAM 4
enum fdcn_lsm_param {
  FDCN_LSM_P_SPOT = 0,
  FDCN_LSM_P_STRIKE,
  FDCN_LSM_P_LOWER, /* lower level (kinds 1, 3, 4, 6)                          */
  FDCN_LSM_P_UPPER  /* upper level (kinds 2, 3, 5, 6)                          */
};
#define FDCN_LSM_NFLAG 3
enum fdcn_lsm_flag {
  FDCN_LSM_F_PUT = 0, /* 0 call, 1 put                                          */
  FDCN_LSM_F_KIND,    /* 0 none, 1 down-out, 2 up-out, 3 double-out, 4 down-in,
                         5 up-in, 6 double-in                                   */
  FDCN_LSM_F_STREAM   /* Philox stream id, 0 .. 2^30 - 1                        */
};
#define FDCN_LSM_NSTEP 9
enum fdcn_lsm_step {
  FDCN_LSM_S_DRIFT = 0, /* (carry - sigma^2 / 2) * dt_m                         */
  FDCN_LSM_S_DIFF,      /* sigma * sqrt(dt_m), > 0                              */
  FDCN_LSM_S_DF_STEP,   /* discount factor over the step, t_m back to t_{m-1}   */
  FDCN_LSM_S_DF_END,    /* discount factor from t_m to valuation                */
  FDCN_LSM_S_MONITOR,   /* 1.0 if t_m is a monitoring time, else 0.0            */
  FDCN_LSM_S_EXERCISE,  /* 1.0 if the holder may exercise at t_m, else 0.0
                           (maturity always exercises)                          */
  FDCN_LSM_S_REBATE,    /* knock-out: paid to a path knocked at t_m; knock-in:
                           read at maturity only                                */
  FDCN_LSM_S_CENTRE,    /* ln(spot) + sum of DRIFT up to m                      */
  FDCN_LSM_S_ISCALE     /* 1 / sqrt(sum of DIFF^2 up to m)                      */
};
#define FDCN_LSM_NSTAT 8
enum fdcn_lsm_stat {
  FDCN_LSM_O_PRICE = 0,  /* mean of the sub-run out-of-sample means             */
  FDCN_LSM_O_STDERR,     /* their sample standard deviation / sqrt(G); 0: G = 1 */
  FDCN_LSM_O_FIT_VALUE,  /* mean of the in-sample means (diagnostic, biased up) */
  FDCN_LSM_O_FIT_STDERR,
  FDCN_LSM_O_SUM,        /* sum of the sub-run out-of-sample means (merging)    */
  FDCN_LSM_O_SUM2,       /* sum of their squares                                */
  FDCN_LSM_O_INVALID,    /* invalid fit steps, over the G sub-runs              */
  FDCN_LSM_O_MIN_MARGIN  /* min |phi - fit(u)| over every fit decision taken,
                            both path sets; +inf if none                        */
};
/* Host pointers; copies in and out on the calling thread's stream and waits. */
int fdcn_mc_lsm_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                      const double* params, const int32_t* flags, const double* step,
                      uint64_t seed, int64_t obs_first, double* stats, double* values_out,
                      double* coef_out);
/* Device pointers, asynchronous on `stream`, no host sync.  `workspace` is
 * device scratch of at least B * ws_bytes_per_contract (fdcn_mc_lsm_plan)
 * bytes -- a smaller workspace_bytes is FDCN_EINVAL -- or NULL: allocated
 * stream-ordered for the call.  The arrays are device memory, so their
 * contents are not checked here: the kernel treats a KIND outside 0..6 as 0. */
int fdcn_mc_lsm_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                          const double* params, const int32_t* flags, const double* step,
                          uint64_t seed, int64_t obs_first, double* stats, double* values_out,
                          double* coef_out, double* workspace, int64_t workspace_bytes,
                          void* stream);
/* Geometry of a launch: observations per sub-run, workspace bytes per
 * contract, doubles per contract of values_out and of coef_out.  Any output
 * pointer may be NULL.  Host only. */
int fdcn_mc_lsm_plan(int32_t n_steps, int32_t G, int32_t antithetic, int32_t* obs_per_subrun,
                     int64_t* ws_bytes_per_contract, int64_t* values_per_contract,
                     int64_t* coef_per_contract);

/* ---- The same with cash dividends on the path.  Everything above holds, and
 *   div [B][n_steps]   cash dividend D_m >= 0 of step m (0.0: none)
 * is one more input.  Within step m the order is: the move x += DRIFT_m +
 * DIFF_m * z_m, then the dividend, then the step's events, all on the
 * ex-dividend spot: the MONITOR test, the exercise decision, the maturity
 * payoff and the regressor u.  A dividend on the last step therefore acts
 * before the maturity payoff.  The dividend map on the spot is
 *   g(s) = s - D  for s >= 2 D,   s / 2  below:
 * continuous, strictly increasing, positive and invertible, with the inverse
 * s + D for s >= D and 2 s below.  On the log-spot, with s = exp(x):
 *   forward  (phases A and C)  x <- log(s - D) if s >= 2 D, else x - ln 2
 *   backward (phase B)         x <- log(s + D) if s >= D,   else x + ln 2
 * each operation rounded separately, ln 2 = 0x1.62e42fefa39efp-1; a step with
 * D_m == 0.0 applies neither.  Phase B walks the fit set backward without
 * storing it: going from t_m to t_{m-1} it first undoes step m's dividend with
 * the inverse map and then subtracts the move.  Because g is continuous at
 * 2 D, a rounding that takes the other branch on the way back (s within
 * rounding of D there) moves x by rounding error only; a clamp such as max(s -
 * D, floor) has no inverse and could not be walked back.  CENTRE_m is the
 * caller's (mc_american.py rolls it through g), ISCALE_m as above.
 * The step table's layout, FDCN_LSM_NSTEP and the workspace (fdcn_mc_lsm_plan)
 * do not change, and a launch with an all-zero div gives the numbers of
 * fdcn_mc_lsm_batch bit for bit.
 * Validation adds (before any device call; FDCN_EINVAL): div NULL; and, host
 * entry only, a dividend that is negative or not finite. */
int fdcn_mc_lsm_div_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                          const double* params, const int32_t* flags, const double* step,
                          const double* div, uint64_t seed, int64_t obs_first, double* stats,
                          double* values_out, double* coef_out);
/* Device pointers, as fdcn_mc_lsm_batch_dev; the contents of div are not
 * checked here. */
int fdcn_mc_lsm_div_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                              const double* params, const int32_t* flags, const double* step,
                              const double* div, uint64_t seed, int64_t obs_first, double* stats,
                              double* values_out, double* coef_out, double* workspace,
                              int64_t workspace_bytes, void* stream);

/* ---- Dual upper bound for the least-squares Monte Carlo (Andersen-Broadie;
 * csrc/fdcn_mc_dual.hip).  The out-of-sample LSM price is a lower bound; the
 * policy it has fitted drives a nested simulation that gives a gap >= 0 with
 * lower bound + gap an upper bound in expectation, whatever the policy.
 * One launch takes B contracts that share n_steps, G, `antithetic`, n_outer
 * and n_inner:
 *   params, flags, step                 those of the fdcn_mc_lsm_batch launch
 *   coef [B][G][n_steps][FDCN_LSM_NCOEF]  what that launch wrote to coef_out:
 *                                       sub-run g's rows are sub-run g's policy
 *   n_outer   outer paths per sub-run, 1 .. FDCN_DUAL_MAX_OUTER
 *   n_inner   inner paths per start, a multiple of 256 (of 512 when
 *             antithetic), up to FDCN_DUAL_MAX_INNER
 *   subrun_first   the absolute number of this launch's sub-run 0 (a shard);
 *             subrun_first + G <= 2^31
 * Steps, events, eligibility and the fitted rule are phase C's above, word for
 * word: on a knock-out a monitored breach is checked first and forces
 * max(phi, REBATE_m); a knock-in path is eligible from its hit step on, that
 * step included; the fitted rule stops on an EXERCISE step before maturity
 * with a valid fit, eligible, phi > 0 and phi > fit(u); maturity always stops.
 * Every cashflow is discounted to valuation: Z_m = phi * DF_END_m is the
 * reward for stopping at m.  Every operation below is rounded separately.
 *
 * Per outer path: x = ln(spot), r = 0, D = -inf; for m = 1 .. n_steps,
 * x += DRIFT_m + DIFF_m * z_m, then
 *   forced stop (knock-out breach at a MONITOR step, or m = n_steps):
 *       D = max(D, 0 - r); the path ends.
 *   the holder may stop (m < n_steps, EXERCISE_m, eligible, phi > 0; the fit
 *   need not be valid): the inner simulation gives C_m, the mean over n_inner
 *   fresh paths started at (x, knocked-in state) of the discounted cashflow of
 *   following phase C's rule from step m + 1 on; then
 *       the fitted rule stops at m:  D = max(D, 0 - r), then r = r + (Z_m - C_m)
 *       otherwise:                   D = max(D, (Z_m - C_m) - r)
 *   any other step (no EXERCISE flag, not eligible, or phi == 0): nothing, and
 *   no inner simulation.  A phi == 0 candidate cannot beat the next stop's,
 *   because C_m >= 0: every cashflow is >= 0, for which REBATE_m >= 0 is
 *   required (a negative one is refused by the host entry).
 * D >= 0 exactly: at the policy's first stop, fitted or forced, r is still 0
 * and the candidate is 0 - 0.  D == 0 for a contract without an EXERCISE step
 * before maturity, and no inner path is run for it.
 * C_m: inner path i of a start is slot k = i / 256 of thread i % 256; each
 * thread adds its slots' cashflows in slot order, a fixed tree v[t] + v[t +
 * off], off = 128 .. 1, adds the threads, and the total is divided by n_inner.
 * The gap of a sub-run is the sum of its D in path order divided by n_outer;
 * a second kernel adds the sub-run gaps in sub-run order.  No floating-point
 * atomics.  A contract's numbers depend on neither B nor its position in the
 * batch.
 *
 * Normals: the Philox mapping of fdcn_mc_lsm_batch with bit 31 of counter word
 * 3 set, so the words are disjoint from the LSM's 2 * id and 2 * id + 1:
 *   outer set  word 2^31 + 2 * id,      o = (subrun_first + g) * n_outer + p,
 *              z_m = element (m - 1) % 2 of pair (m - 1) / 2
 *   inner set  word 2^31 + 2 * id + 1,
 *              o = ((((subrun_first + g) * 2^10 + p) * 2^9 + (m - 1)) * 2^14 + j
 *              for observation j of the start at step m of outer path p: 31 +
 *              10 + 9 + 14 = 64 bits at the caps, and injective; step m + 1 + t
 *              of the inner path draws element t % 2 of pair t / 2.
 * Without antithetic inner path i is observation i; with it a start has
 * n_inner / 2 observations and path i is observation (k / 2) * 256 + i % 256
 * with +z for k even and -z for k odd, as in the LSM.  The outer paths are not
 * paired.  Disjoint sub-run ranges of one (seed, stream id) are shards of one
 * run: their (G, sum, sum of squares) of the sub-run gaps merge.
 *   stats [B][FDCN_DUAL_NSTAT]          see enum fdcn_dual_stat
 *   gap_out  [B][G * n_outer]           D per outer path (NULL: none)
 *   cont_out [B][G * n_outer][n_steps]  C_m, 0.0 where no inner simulation was
 *                                       run (NULL: none)
 * Cash dividends: there is no `div` input here; fdcn_mc_lsm_dual_div_batch
 * below takes one.
 * Validation (before any device call; FDCN_EINVAL): that of fdcn_mc_lsm_batch
 * with subrun_first in the place of obs_first, and n_outer or n_inner out of
 * range, NULL coef, and, host entry only, a negative REBATE on a barrier
 * contract or a coefficient that is not finite. */
#define FDCN_DUAL_MAX_OUTER 1024
#define FDCN_DUAL_MAX_INNER 16384
#define FDCN_DUAL_NSTAT 7
enum fdcn_dual_stat {
  FDCN_DUAL_O_GAP = 0,     /* mean of the sub-run gaps                            */
  FDCN_DUAL_O_STDERR,      /* their sample standard deviation / sqrt(G); 0: G = 1 */
  FDCN_DUAL_O_SUM,         /* sum of the sub-run gaps (merging)                   */
  FDCN_DUAL_O_SUM2,        /* sum of their squares                                */
  FDCN_DUAL_O_MIN_MARGIN,  /* min |phi - fit(u)| over every fitted decision taken,
                              outer and inner; +inf if none                       */
  FDCN_DUAL_O_INNER_PATHS, /* inner paths run: starts * n_inner                   */
  FDCN_DUAL_O_INNER_STEPS  /* steps those paths walked until they stopped         */
};
/* Host pointers; copies in and out on the calling thread's stream and waits. */
int fdcn_mc_lsm_dual_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                           int32_t n_outer, int32_t n_inner, const double* params,
                           const int32_t* flags, const double* step, const double* coef,
                           uint64_t seed, int64_t subrun_first, double* stats, double* gap_out,
                           double* cont_out);
/* Device pointers, asynchronous on `stream`, no host sync; `workspace` as in
 * fdcn_mc_lsm_batch_dev, sized by fdcn_mc_lsm_dual_plan, or NULL.  The
 * contents of the arrays are not checked here. */
int fdcn_mc_lsm_dual_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                               int32_t n_outer, int32_t n_inner, const double* params,
                               const int32_t* flags, const double* step, const double* coef,
                               uint64_t seed, int64_t subrun_first, double* stats,
                               double* gap_out, double* cont_out, double* workspace,
                               int64_t workspace_bytes, void* stream);
/* Geometry of a launch: workspace bytes per contract, doubles per contract of
 * gap_out and of cont_out.  Any output pointer may be NULL.  Host only. */
int fdcn_mc_lsm_dual_plan(int32_t n_steps, int32_t G, int32_t antithetic, int32_t n_outer,
                          int32_t n_inner, int64_t* ws_bytes_per_contract,
                          int64_t* gap_per_contract, int64_t* cont_per_contract);

/* ---- The same with cash dividends on the path: the contract of
 * fdcn_mc_lsm_dual_batch with one more input,
 *   div [B][n_steps]   cash dividend D_m >= 0 of step m (0.0: none),
 * the row of the fdcn_mc_lsm_div_batch launch that wrote coef.  Both walks go
 * forward only, so they need the map g of fdcn_mc_lsm_div_batch and never its
 * inverse.  Within step m, on the outer walk and on every inner walk, the order
 * is:
 *   1. the move x += DRIFT_m + DIFF_m * z_m;
 *   2. the dividend, when D_m != 0.0: with s = exp(x),
 *      x <- log(s - D_m) if s >= 2 D_m, else x - ln 2, each operation rounded
 *      separately, ln 2 = 0x1.62e42fefa39efp-1;
 *   3. the step's events on the ex-dividend spot: the MONITOR test, the fitted
 *      rule's decision and its regressor u, the maturity payoff, and the
 *      candidate of the step with the start state (x, knocked-in state) of its
 *      inner simulation.
 * A step with a dividend and no flag still pays it, on inner paths too: a path
 * that is still alive takes the dividend before anything asks whether the step
 * has an event.  The inner simulation of a start at step m begins with the move
 * of step m + 1, so step m's dividend is in its start state and is not paid
 * again.  Streams, the observation packing, the sums, the tree, stats, gap_out
 * and cont_out are unchanged, fdcn_mc_lsm_dual_plan serves both forms, and a
 * launch with an all-zero div gives the numbers of fdcn_mc_lsm_dual_batch bit
 * for bit.  D >= 0 holds as before: g does not enter the argument.
 * Validation adds (before any device call; FDCN_EINVAL): div NULL; and, host
 * entry only, a dividend that is negative or not finite. */
int fdcn_mc_lsm_dual_div_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                               int32_t n_outer, int32_t n_inner, const double* params,
                               const int32_t* flags, const double* step, const double* div,
                               const double* coef, uint64_t seed, int64_t subrun_first,
                               double* stats, double* gap_out, double* cont_out);
/* Device pointers, as fdcn_mc_lsm_dual_batch_dev; the contents of div are not
 * checked here. */
int fdcn_mc_lsm_dual_div_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                                   int32_t n_outer, int32_t n_inner, const double* params,
                                   const int32_t* flags, const double* step, const double* div,
                                   const double* coef, uint64_t seed, int64_t subrun_first,
                                   double* stats, double* gap_out, double* cont_out,
                                   double* workspace, int64_t workspace_bytes, void* stream);

/* ---- Monte Carlo bounds under a given exercise table (csrc/fdcn_mc_policy.hip,
 * csrc/fdcn_mc_policy.h).  The least-squares Monte Carlo fits its stopping
 * rule; here the rule is an input, for instance the exercise boundary of a
 * Bermudan FD pricer (mc_american.policy_from_pricer).  Any rule gives a lower
 * bound and any rule gives a dual upper bound, so a wrong table shows as a low
 * lower bound and a wide gap, never as agreement.  Additive: FDCN_ABI_VERSION
 * is still 8.
 *   params, flags, step                 as in fdcn_mc_lsm_batch
 *   policy [B][n_steps][FDCN_POLICY_NCOL]  row m - 1 is step m: X_LO_m, X_HI_m,
 *                                       a band in the log-spot.  Per contract,
 *                                       not per sub-run.
 * The table rule replaces phase C's fitted rule.  It stops a path at step m
 * when all of these hold: m < n_steps; EXERCISE_m != 0; the path is eligible;
 * X_LO_m <= x <= X_HI_m, both ends inclusive; phi > 0.  +-inf are legal
 * entries, X_LO_m > X_HI_m means never at that step, and a row on a step
 * without an EXERCISE flag is ignored.  Everything else is phase C word for
 * word: the move x += DRIFT_m + DIFF_m * z_m; on a knock-out a monitored
 * breach is checked first and pays max(phi, REBATE_m); a knock-in path is
 * eligible from its hit step on, that step included; maturity always stops;
 * the value is the cashflow times DF_END_m; every operation is rounded
 * separately.  The band is compared in x, so exp(x) is evaluated only on a
 * MONITOR step of a barrier contract, for an in-band decision and at maturity.
 * A rule decision is taken for every path that is alive and eligible at an
 * EXERCISE step m < n_steps, whatever its phi (phi is read in band only);
 * MIN_MARGIN is the smallest distance |x - X_LO_m|, |x - X_HI_m| to a finite
 * entry over those decisions: no decision of a run can flip under a
 * perturbation of x smaller than it.
 * Cash dividends: there is no `div` input here; fdcn_mc_policy_div_batch and
 * fdcn_mc_policy_dual_div_batch below take one.
 *
 * Lower bound, fdcn_mc_policy_batch.  The paths are the LSM's price set:
 * counter word 3 = 2 * stream id + 1, the observation mapping, the antithetic
 * pairing by slot parity, FDCN_LSM_SUBRUN paths per sub-run, one workgroup of
 * 256 threads per (contract, sub-run) and obs_first as in fdcn_mc_lsm_batch,
 * so values_out of the two entries pair path for path.  The reduction is the
 * LSM's too: per thread in slot order, the fixed tree v[t] + v[t + off], off =
 * 128 .. 1, one partial per sub-run, added in sub-run order by a second kernel;
 * no floating-point atomics.  With a table that never stops, PRICE, STDERR,
 * SUM, SUM2 and values_out are those of fdcn_mc_lsm_batch on the contract
 * with its EXERCISE flags cleared, bit for bit.
 *   stats [B][FDCN_POLICY_NSTAT]        see enum fdcn_policy_stat
 *   values_out [B][G * FDCN_LSM_SUBRUN] value per path (NULL: none)
 * Validation (before any device call; FDCN_EINVAL): all of fdcn_mc_lsm_batch,
 * NULL policy, and, host entry only, a NaN in policy. */
#define FDCN_POLICY_NCOL 2
enum fdcn_policy_col {
  FDCN_POLICY_X_LO = 0, /* stop only where x >= X_LO_m (-inf: no lower end)    */
  FDCN_POLICY_X_HI      /* stop only where x <= X_HI_m (+inf: no upper end)    */
};
#define FDCN_POLICY_NSTAT 6
enum fdcn_policy_stat {
  FDCN_POLICY_O_PRICE = 0,  /* mean of the sub-run means                          */
  FDCN_POLICY_O_STDERR,     /* their sample standard deviation / sqrt(G); 0: G = 1 */
  FDCN_POLICY_O_SUM,        /* sum of the sub-run means (merging)                 */
  FDCN_POLICY_O_SUM2,       /* sum of their squares                               */
  FDCN_POLICY_O_MIN_MARGIN, /* min distance of x to a finite X_LO_m / X_HI_m over
                               the rule decisions taken; +inf if none            */
  FDCN_POLICY_O_EXERCISED   /* paths the rule stopped (an exact integer)          */
};
/* Host pointers; copies in and out on the calling thread's stream and waits. */
int fdcn_mc_policy_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                         const double* params, const int32_t* flags, const double* step,
                         const double* policy, uint64_t seed, int64_t obs_first, double* stats,
                         double* values_out);
/* Device pointers, asynchronous on `stream`, no host sync; `workspace` as in
 * fdcn_mc_lsm_batch_dev, sized by fdcn_mc_policy_plan, or NULL.  The contents
 * of the arrays are not checked here. */
int fdcn_mc_policy_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                             const double* params, const int32_t* flags, const double* step,
                             const double* policy, uint64_t seed, int64_t obs_first,
                             double* stats, double* values_out, double* workspace,
                             int64_t workspace_bytes, void* stream);
/* Geometry of a launch: observations per sub-run, workspace bytes per
 * contract, doubles per contract of values_out.  Any output pointer may be
 * NULL.  Host only. */
int fdcn_mc_policy_plan(int32_t n_steps, int32_t G, int32_t antithetic, int32_t* obs_per_subrun,
                        int64_t* ws_bytes_per_contract, int64_t* values_per_contract);
/* The same with cash dividends on the path: one more input,
 *   div [B][n_steps]   cash dividend D_m >= 0 of step m (0.0: none).
 * Within step m the order is: the move x += DRIFT_m + DIFF_m * z_m; then the
 * dividend, when D_m != 0.0, through the forward map of fdcn_mc_lsm_div_batch
 * (x <- log(exp(x) - D_m) if exp(x) >= 2 D_m, else x - ln 2); then the step's
 * events on the ex-dividend spot: the MONITOR test, the band decision in x and
 * the maturity payoff.  A step with a dividend and no flag still pays it.  A
 * dividend step evaluates exp and log once for the map; elsewhere the spot is
 * read only where stated above.  With a table that never stops, PRICE, STDERR,
 * SUM, SUM2 and values_out are those of fdcn_mc_lsm_div_batch on the contract
 * with its EXERCISE flags cleared, bit for bit; with an all-zero div every
 * output is that of fdcn_mc_policy_batch, bit for bit.  fdcn_mc_policy_plan
 * serves both forms.
 * Validation adds (before any device call; FDCN_EINVAL): div NULL; and, host
 * entry only, a dividend that is negative or not finite. */
int fdcn_mc_policy_div_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                             const double* params, const int32_t* flags, const double* step,
                             const double* div, const double* policy, uint64_t seed,
                             int64_t obs_first, double* stats, double* values_out);
int fdcn_mc_policy_div_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                                 const double* params, const int32_t* flags, const double* step,
                                 const double* div, const double* policy, uint64_t seed,
                                 int64_t obs_first, double* stats, double* values_out,
                                 double* workspace, int64_t workspace_bytes, void* stream);

/* Upper bound, fdcn_mc_policy_dual_batch: the contract of
 * fdcn_mc_lsm_dual_batch with policy [B][n_steps][FDCN_POLICY_NCOL] in the
 * place of coef.  The outer and inner streams (bit 31 words), the observation
 * packing, the limits of n_outer and n_inner, FDCN_DUAL_NSTAT, gap_out and
 * cont_out are unchanged.  A candidate arises at every EXERCISE step m <
 * n_steps at which the outer path is eligible with phi > 0; "the rule stops
 * at m" is X_LO_m <= x <= X_HI_m, for the outer and the inner walks alike.
 * MIN_MARGIN is the x-distance defined above, over the decisions of outer and
 * inner paths.  With a table that never stops, every output is that of
 * fdcn_mc_lsm_dual_batch with an all-zero coef, bit for bit.
 * Validation: that of fdcn_mc_lsm_dual_batch with policy in the place of coef;
 * host entry only, a NaN in policy. */
int fdcn_mc_policy_dual_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                              int32_t n_outer, int32_t n_inner, const double* params,
                              const int32_t* flags, const double* step, const double* policy,
                              uint64_t seed, int64_t subrun_first, double* stats,
                              double* gap_out, double* cont_out);
int fdcn_mc_policy_dual_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                                  int32_t n_outer, int32_t n_inner, const double* params,
                                  const int32_t* flags, const double* step,
                                  const double* policy, uint64_t seed, int64_t subrun_first,
                                  double* stats, double* gap_out, double* cont_out,
                                  double* workspace, int64_t workspace_bytes, void* stream);
int fdcn_mc_policy_dual_plan(int32_t n_steps, int32_t G, int32_t antithetic, int32_t n_outer,
                             int32_t n_inner, int64_t* ws_bytes_per_contract,
                             int64_t* gap_per_contract, int64_t* cont_per_contract);
/* The same with cash dividends on the path: div [B][n_steps] as in
 * fdcn_mc_policy_div_batch, and the order within a step of
 * fdcn_mc_lsm_dual_div_batch on the outer walk and on every inner walk: the
 * move, the dividend (a step without a flag pays it too), then the MONITOR
 * test, the band decision in x, the maturity payoff and the candidate with the
 * start state of its inner simulation, all on the ex-dividend spot.  With a
 * table that never stops, every output is that of fdcn_mc_lsm_dual_div_batch
 * with an all-zero coef, bit for bit; with an all-zero div, that of
 * fdcn_mc_policy_dual_batch.  fdcn_mc_policy_dual_plan serves both forms.
 * Validation adds: div NULL; and, host entry only, a dividend that is negative
 * or not finite. */
int fdcn_mc_policy_dual_div_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                                  int32_t n_outer, int32_t n_inner, const double* params,
                                  const int32_t* flags, const double* step, const double* div,
                                  const double* policy, uint64_t seed, int64_t subrun_first,
                                  double* stats, double* gap_out, double* cont_out);
int fdcn_mc_policy_dual_div_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                                      int32_t n_outer, int32_t n_inner, const double* params,
                                      const int32_t* flags, const double* step,
                                      const double* div, const double* policy, uint64_t seed,
                                      int64_t subrun_first, double* stats, double* gap_out,
                                      double* cont_out, double* workspace,
                                      int64_t workspace_bytes, void* stream);

/* ---- host-side plan helpers (no device) -------------------------------- */
/* Uniform log grid of the pricers' _build_log_grid
 * (discrete_barrier_fdm_pricer.py:342-364, fd_american_equity.py:363-384):
 *   x[i] = x_min + (double)i * dx,   s[i] = exp(x[i]),   i = 0..n
 * with the C library's exp (the one CPython's math.exp calls), so the nodes
 * are bit-identical to the reference's list comprehensions.  x may be NULL.
 * Returns FDCN_OK or FDCN_EINVAL (n < 0, s NULL). */
int fdcn_log_grid(double x_min, double dx, int32_t n, double* x, double* s);

/* The accumulated tau of FDCN_I_TAU_MODE = 1, as the kernels evaluate it:
 * tau[m] = tau after step m of `tau = tau + dt` starting from tau0
 * (fd_american_equity.py:664-724), m = 0..n-1.  Bit-identical to the serial
 * adds; the device evaluates it in constant-increment runs (one per binade
 * plus single steps at binade crossings and rounding ties) instead of n
 * dependent adds.  fdcn_tau_runs returns the number of runs.  Host only. */
int fdcn_tau_sequence(double tau0, double dt, int32_t n, double* tau);
int fdcn_tau_runs(double tau0, double dt, int32_t n);

/* Discrete-dividend jump between two American segments
 * (AmericanFDMPricer._apply_dividend_jump, fd_american_equity.py:732-772,
 * with the natural cubic spline of :479-553):
 *   q_i = s_i - cash_div,  V_out[i] = v[0] if q_i <= s[0], v[n-1] if q_i >= s[n-1],
 *   else spline(q_i);  calls (strike_call >= 0): V_out[i] = max(V_out[i], max(s_i - K, 0)).
 * Same operation order as the reference, so the result is bit-identical.
 * s strictly increasing, n >= 2.  Host only (no device). */
int fdcn_dividend_jump(int32_t n, const double* s, const double* v, double cash_div,
                       double strike_call, double* v_out);

/* ---- whole-file plan builder (finite_difference_amd/csrc/fdcn_plan.hip) --
 * The discrete-barrier scenario runner's per-row work (run_config_scenarios.py
 * :137-195 over DiscreteBarrierFDMPricer: choose_grid_parameters, the log
 * grid, payoff, boundaries, knock-out thresholds, monitoring rebates and the
 * operator coefficients of the base and sigma-bumped solves, …pricer.py
 * :270-547, :883-904) for R rows at once, with libm's exp/log/sqrt and the
 * reference's operation order: the plan arrays are bit-identical to the
 * per-row facade's.  Output solve q = 2*row + (0 base, 1 bumped by dv_sigma):
 *   params [2R][FDCN_NPARAM], iparams [2R][FDCN_NIPARAM] (monitor run q*n_mon),
 *   v_init [2R][N] (N = the grid's N_s, the march's n_nodes: *n_nodes_out),
 *   mon_rebate [2R][n_mon] (steps: mon_k, shared by all rows),
 *   rint / rdbl [2R] readouts in fdcn_session_greeks layout (slot field = q),
 *   tparams [R][FDCN_GK_NPARAM] (FDCN_GK_BARRIER, readouts 2*row, 2*row+1).
 * v_init holds 2R * n_nodes_cap doubles; FDCN_EINVAL (nothing written) if
 * N > n_nodes_cap or the rows' N differ (parity mode N = ceil(k_tail n_time)
 * up to rounding, explicit mode N = n_space).  grid_mode 0 parity, 1 explicit. */
#define FDCN_BP_NROW 10
enum fdcn_bp_row {
  FDCN_BP_SPOT = 0, FDCN_BP_STRIKE, FDCN_BP_SIGMA, FDCN_BP_LO, FDCN_BP_UP,
  FDCN_BP_CARRY, FDCN_BP_DIVY, FDCN_BP_DISC, FDCN_BP_PV, FDCN_BP_REBATE
};
#define FDCN_BP_NFLAG 4
enum fdcn_bp_flag {
  FDCN_BP_PUT = 0, /* 1 for puts */
  FDCN_BP_KO,      /* 1 down-and-out, 2 up-and-out, 3 double-out (knock-ins: their twin) */
  FDCN_BP_HAS_LO, FDCN_BP_HAS_UP
};
int fdcn_barrier_plan(int32_t R, const double* row, const int32_t* rflag, double T,
                      int32_t n_space, int32_t n_time, int32_t grid_mode, int32_t n_nodes_cap,
                      double k_tail, double dv_sigma, int32_t rebate_at_hit, int32_t n_mon,
                      const int32_t* mon_k, double* params, int32_t* iparams, double* v_init,
                      double* mon_rebate, int32_t* rint, double* rdbl, double* tparams,
                      int32_t* n_nodes_out);
/* American counterpart (run_american_scenarios.py:209-277 over
 * AmericanFDMPricer, fd_american_equity.py:340-448, :855-907): the log grid
 * of one (row, sigma) job each -- band around sqrt(S K), uniform log nodes,
 * spot and strike snapped to the nearest node, payoff with the snapped
 * strike, operator coefficients (q = 0), Dirichlet forms, TAU_MODE 1 -- and
 * its two readouts at the snapped spot.  n_space + 1 nodes per job.
 *   job [J][FDCN_AP_NJOB] = spot, strike, sigma, carry, r;  call [J] (1 call, 0 put)
 *   params [J][FDCN_NPARAM]: DT and TAU0 left 0 (set per segment by the caller)
 *   iparams [J][FDCN_NIPARAM], payoff [J][n_space+1], s_nodes [J][n_space+1]
 *   (may be NULL), rint / rdbl [2J]: row 2q the interpolation readout, row
 *   2q+1 with the cubic Delta/Gamma (fdcn_session_greeks layout, slot = q),
 *   gout [J][FDCN_AP_NOUT] = snapped spot, snapped strike, dx, spot index. */
#define FDCN_AP_NJOB 5
enum fdcn_ap_job { FDCN_AP_SPOT = 0, FDCN_AP_STRIKE, FDCN_AP_SIGMA, FDCN_AP_CARRY, FDCN_AP_DISC };
#define FDCN_AP_NOUT 4
int fdcn_american_plan(int32_t J, const double* job, const int32_t* call, int32_t n_space,
                       double s_max_mult, double T, double* params, int32_t* iparams,
                       double* payoff, double* s_nodes, int32_t* rint, double* rdbl,
                       double* gout);
/* y = exp(x) (op 0), log(x) (1), sqrt(x) (2), pow(x, 2.0) (3) elementwise with
 * the C library (the functions CPython's math module and float ** call). */
int fdcn_vmath(int32_t op, int64_t n, const double* x, double* y);

const char* fdcn_last_error(void);
int fdcn_device_count(void);   /* gfx950 devices visible; 0 if none          */
/* The HIP ordinals of the visible gfx950 devices, ascending, into ord[cap];
 * returns how many there are (may exceed cap), 0 if none.  On a host with
 * other GPUs too, local rank k binds ord[k], not HIP ordinal k. */
int fdcn_device_ordinals(int32_t* ord, int32_t cap);
int fdcn_abi_version(void);    /* FDCN_ABI_VERSION                           */
/* Make `ordinal` the calling thread's current HIP device (hipSetDevice): the
 * host-pointer entry points run there.  One process per GPU calls it once
 * with its local rank.  Returns FDCN_OK or FDCN_EINVAL / FDCN_EHIP. */
int fdcn_select_device(int32_t ordinal);
int fdcn_current_device(void); /* the calling thread's device, or < 0 on error */

#ifdef __cplusplus
}
#endif

#endif /* FDCN_H */
