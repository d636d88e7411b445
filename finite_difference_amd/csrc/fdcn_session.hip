// fdcn_session.hip -- device-resident march sessions (C ABI: include/fdcn.h).
//
// The host-array entry points (fdcn_cn_batch / fdcn_it_batch) copy every
// value vector back to the host.  The pricers need far less: the reference
// reads 3-4 nodes per solve for price/Delta/Gamma (discrete_barrier_fdm_pricer.py
// :629-646, :949-978; fd_american_equity.py:855-907), combines solves into
// vega / theta / Richardson (:883-904, :970-1068), and between the dividend
// segments of an American solve remaps the whole vector through a natural
// cubic spline (fd_american_equity.py:479-553, :732-772, :825-843).  A session
// keeps the value vectors in HBM ("slots") and chains those steps on the
// device:
//
//   fdcn_session_march          one batched CN/KO or IT launch; initial vectors
//                               from the host or from earlier slots
//   fdcn_session_march_ps       the IT march with its payoff in earlier slots
//   fdcn_session_upload         host vectors into slots (a chain's payoff, once)
//   fdcn_session_dividend_jump  spline remap of slots into new slots (device)
//   fdcn_session_knockout       monitoring-date knock-out of slots, in place
//   fdcn_session_knockin        monitoring-date knock-in: masked copy from other
//                               slots (the coupled American chain), in place
//   fdcn_session_exercise       exercise date of a Bermudan chain: max(V, floor)
//                               fused with the knock-out, in place; records
//                               the exercise region of each vector
//   fdcn_session_exercise_regions  those records back to the host
//   fdcn_session_greeks        per-trade readouts + combinations -> T x 6
//                               scalars back to the host
//   fdcn_session_fetch          whole vectors back (when a caller wants them)
//
// Each march runs on one of a few session streams (independent launch groups
// overlap -- the American N / 2N pair); a consumer of slots waits on the
// events of the launches that produced them.  Host inputs are staged through a
// session-owned pinned arena, so every copy is truly asynchronous and the
// caller's arrays are free to go as soon as a call returns.  Device memory is
// stream-ordered (hipMallocAsync from the device pool) and released by
// fdcn_session_destroy.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../include/fdcn.h"
#include "fdcn_session_book.h"
#include "fdcn_shared.h"

namespace {

// Staging copy into pinned memory: whole-file plans stage 100-400 MB of
// initial vectors per march, which one thread copies at ~8 GB/s; above 16 MB
// the copy is split over up to 8 host threads.
void stage_copy(void* dst, const void* src, size_t n) {
  constexpr size_t kPar = size_t(16) << 20;
  if (n < kPar) {
    memcpy(dst, src, n);
    return;
  }
  unsigned hw = std::thread::hardware_concurrency();
  const size_t nt = std::min<size_t>(hw ? hw : 1, 8);
  const size_t chunk = (n / nt + 4095) & ~size_t(4095);
  std::vector<std::thread> th;
  for (size_t t = 0; t < nt; ++t) {
    const size_t a = t * chunk;
    if (a >= n) break;
    const size_t len = std::min(chunk, n - a);
    th.emplace_back([=]() { memcpy((char*)dst + a, (const char*)src + a, len); });
  }
  for (auto& x : th) x.join();
}

int sfail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return fdcn_internal::set_error(code, buf);
}

#define S_TRY(expr)                                                                \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) return sfail(FDCN_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

constexpr int kMaxStreams = 4;
using fdcn_book::al256;
using fdcn_book::Layout;

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// v_init rows from earlier slots: row b <- *src[b] (n doubles)
__global__ void gather_rows(const uint64_t* __restrict__ src, double* __restrict__ dst, int n) {
  const double* s = reinterpret_cast<const double*>(src[blockIdx.x]);
  double* d = dst + (size_t)blockIdx.x * n;
  for (int i = threadIdx.x; i < n; i += blockDim.x) d[i] = s[i];
}

// Knock-out event between two segments of an American march: on the knocked
// nodes (j <= ko_lo or j >= ko_hi) of vector b, V_j <- max(floor_j, R_b), or
// V_j <- R_b without a floor; every other node is left alone.  Threads run
// along the nodes (`chunks` workgroups of 256 per vector, one launch for the
// batch), so the floor loads and the stores are contiguous 8-byte accesses.
// max keeps the floor on ties and passes its NaN on, as np.maximum(floor, R).
__global__ void __launch_bounds__(256)
knockout_kernel(int n, int chunks, const uint64_t* __restrict__ dst,
                const uint64_t* __restrict__ floor_src, const int32_t* __restrict__ ko_lo,
                const int32_t* __restrict__ ko_hi, const double* __restrict__ rebate) {
  const int b = blockIdx.x / chunks;
  const int j = (blockIdx.x % chunks) * 256 + threadIdx.x;
  if (j >= n || (j > ko_lo[b] && j < ko_hi[b])) return;
  double x = rebate[b];
  if (floor_src) {
    const double f = reinterpret_cast<const double*>(floor_src[b])[j];
    x = (f >= x || f != f) ? f : x;
  }
  reinterpret_cast<double*>(dst[b])[j] = x;
}

// Knock-in event that couples two chains of an American knock-in march: on
// the knocked nodes (j <= ko_lo or j >= ko_hi) of vector b, V_j <- src_j with
// src the vector of another slot (the vanilla American value the holder owns
// once the barrier is seen breached); every other node is left alone.  Same
// shape as knockout_kernel: threads along the nodes, `chunks` workgroups of
// 256 per vector, contiguous 8-byte loads and stores.  The value moves as 64
// bits, so NaN payloads and signed zeros arrive as they are.
__global__ void __launch_bounds__(256)
knockin_kernel(int n, int chunks, const uint64_t* __restrict__ dst,
               const uint64_t* __restrict__ src, const int32_t* __restrict__ ko_lo,
               const int32_t* __restrict__ ko_hi) {
  const int b = blockIdx.x / chunks;
  const int j = (blockIdx.x % chunks) * 256 + threadIdx.x;
  if (j >= n || (j > ko_lo[b] && j < ko_hi[b])) return;
  reinterpret_cast<uint64_t*>(dst[b])[j] = reinterpret_cast<const uint64_t*>(src[b])[j];
}

// Exercise event of a Bermudan march, fused with the knock-out of a date that
// is also monitored: on the knocked nodes (j <= ko_lo or j >= ko_hi; none when
// ko_lo == NULL) of vector b, V_j <- max(floor_j, R_b); on every other node
// V_j <- max(V_j, floor_j).  Both max pass a NaN of either operand on and keep
// the first operand on ties, as np.maximum(floor, R) and np.maximum(V, floor).
// One workgroup of 256 threads per vector strides along the nodes (contiguous
// 8-byte accesses; a node is stored only where its value changes).  Each
// thread keeps (min j, max j, count) of its nodes that are not knocked and
// have floor_j > V_j (a NaN compares false): the exercise region.  The three
// are reduced by shuffles within each wave of 64 and across the four waves
// through LDS, and thread 0 stores them to region[b][0..2]: no atomics, so
// the record does not depend on timing.  Empty region: (n, -1, 0).
__global__ void __launch_bounds__(256)
exercise_kernel(int n, const uint64_t* __restrict__ dst, const uint64_t* __restrict__ floor_src,
                const int32_t* __restrict__ ko_lo, const int32_t* __restrict__ ko_hi,
                const double* __restrict__ rebate, int32_t* __restrict__ region) {
  __shared__ int32_t part[4][3];
  const int b = blockIdx.x;
  double* v = reinterpret_cast<double*>(dst[b]);
  const double* f = reinterpret_cast<const double*>(floor_src[b]);
  int lo = -1, hi = n;
  double R = 0.0;
  if (ko_lo) {
    lo = ko_lo[b];
    hi = ko_hi[b];
    R = rebate[b];
  }
  int mn = n, mx = -1, cnt = 0;
  for (int j = threadIdx.x; j < n; j += 256) {
    const double fj = f[j];
    if (j <= lo || j >= hi) {
      v[j] = (fj >= R || fj != fj) ? fj : R;
      continue;
    }
    const double vj = v[j];
    if (fj > vj) {
      mn = min(mn, j);
      mx = j;  // j grows along the stride
      ++cnt;
    }
    if (!(vj >= fj || vj != vj)) v[j] = fj;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    mn = min(mn, __shfl_down(mn, (unsigned)d, 64));
    mx = max(mx, __shfl_down(mx, (unsigned)d, 64));
    cnt += __shfl_down(cnt, (unsigned)d, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[w][0] = mn;
    part[w][1] = mx;
    part[w][2] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) {
      mn = min(mn, part[k][0]);
      mx = max(mx, part[k][1]);
      cnt += part[k][2];
    }
    region[3 * b + 0] = mn;
    region[3 * b + 1] = mx;
    region[3 * b + 2] = cnt;
  }
}

// Dividend jump of one value vector per workgroup (fd_american_equity.py
// :732-772 with the natural cubic spline of :479-553).  Lane 0 runs the
// spline's tridiagonal sweep (the same operation order as the reference and
// as fdcn_dividend_jump, contraction off, IEEE division: bit-identical);
// then all lanes evaluate V(S - D) at their nodes (binary search for the
// interval, as searchsorted(side="right") - 1).
__global__ void __launch_bounds__(64)
dividend_jump_kernel(int n, const uint64_t* __restrict__ src, const double* __restrict__ s_all,
                     const double* __restrict__ cash, const double* __restrict__ strike,
                     double* __restrict__ out_all, double* __restrict__ work) {
#pragma clang fp contract(off)
  const int b = blockIdx.x;
  const double* v = reinterpret_cast<const double*>(src[b]);
  const double* s = s_all + (size_t)b * n;
  double* out = out_all + (size_t)b * n;
  double* mu = work + (size_t)b * 3 * n;
  double* z = mu + n;
  double* c = z + n;
  if (threadIdx.x == 0) {
    mu[0] = 0.0;
    z[0] = 0.0;
    for (int i = 1; i + 1 < n; ++i) {
      const double hm = s[i] - s[i - 1], h = s[i + 1] - s[i];
      const double alpha = 3.0 / h * (v[i + 1] - v[i]) - 3.0 / hm * (v[i] - v[i - 1]);
      const double l = 2.0 * (s[i + 1] - s[i - 1]) - hm * mu[i - 1];
      mu[i] = h / l;
      z[i] = (alpha - hm * z[i - 1]) / l;
    }
    c[n - 1] = 0.0;
    z[n - 1] = 0.0;
    mu[n - 1] = 0.0;
    for (int j = n - 2; j >= 0; --j) c[j] = z[j] - mu[j] * c[j + 1];
  }
  __syncthreads();
  const double D = cash[b], K = strike[b];
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double q = s[i] - D;
    double cont;
    if (q <= s[0]) {
      cont = v[0];
    } else if (q >= s[n - 1]) {
      cont = v[n - 1];
    } else {
      int lo = 0, hi = n;  // first index with s[idx] > q
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s[mid] > q) hi = mid;
        else lo = mid + 1;
      }
      int j = lo - 1;
      if (j > n - 2) j = n - 2;
      const double h = s[j + 1] - s[j];
      const double bj = (v[j + 1] - v[j]) / h - h * (c[j + 1] + 2.0 * c[j]) / 3.0;
      const double dj = (c[j + 1] - c[j]) / (3.0 * h);
      const double t = q - s[j];
      cont = v[j] + bj * t + c[j] * t * t + dj * t * t * t;
    }
    if (K >= 0.0) {  // calls may exercise at the ex-date: max(cont, payoff)
      const double e = s[i] - K;
      const double ex = (0.0 > e) ? 0.0 : e;
      cont = (ex > cont) ? ex : cont;
    }
    out[i] = cont;
  }
}

// ---- Greeks epilogue -------------------------------------------------------
// Readout r of a value vector (ints [slot, interp_case, ilo, idx, dg_mode] are
// resolved on the host into an address; doubles [S_i, s_lo, s_hi, S_d, s_a,
// s_b, s_c, s_d]):
//   price  linear interpolation at S_i (…pricer.py:629-646, equity.py:855-874):
//          interp_case 1 -> V[0], 2 -> V[ilo], else (1-w) V[ilo] + w V[ilo+1],
//          w = (S_i - s_lo) / (s_hi - s_lo)
//   dg_mode 1  non-uniform 3-point Delta/Gamma at idx (…pricer.py:949-978)
//           2  local cubic through idx-1..idx+2 in z = s - S_d, Delta = c,
//              Gamma = 2b (fd_american_equity.py:876-907)
struct Readout {
  double price, delta, gamma;
};

__device__ Readout read_grid(const double* V, const int32_t* ri, const double* rd) {
#pragma clang fp contract(off)
  Readout o{0.0, 0.0, 0.0};
  const int icase = ri[1], ilo = ri[2], idx = ri[3], mode = ri[4];
  if (icase == 1) o.price = V[0];
  else if (icase == 2) o.price = V[ilo];
  else {
    const double w = (rd[0] - rd[1]) / (rd[2] - rd[1]);
    o.price = (1.0 - w) * V[ilo] + w * V[ilo + 1];
  }
  if (mode == 1) {
    const double h1 = rd[5] - rd[4], h2 = rd[6] - rd[5];
    const double Vm = V[idx - 1], V0 = V[idx], Vp = V[idx + 1];
    o.delta = -h2 / (h1 * (h1 + h2)) * Vm + (h2 - h1) / (h1 * h2) * V0 + h1 / (h2 * (h1 + h2)) * Vp;
    o.gamma = 2.0 * (Vm / (h1 * (h1 + h2)) - V0 / (h1 * h2) + Vp / (h2 * (h1 + h2)));
  } else if (mode == 2) {
    // [z^3 z^2 z 1] coef = y, LU with partial pivoting (LAPACK dgetf2 order)
    double A[4][4], y[4];
    for (int k = 0; k < 4; ++k) {
      const double zk = rd[4 + k] - rd[3];
      A[k][0] = zk * zk * zk;
      A[k][1] = zk * zk;
      A[k][2] = zk;
      A[k][3] = 1.0;
      y[k] = V[idx - 1 + k];
    }
    int perm[4] = {0, 1, 2, 3};
    for (int j = 0; j < 4; ++j) {
      int p = j;
      for (int i = j + 1; i < 4; ++i)
        if (fabs(A[i][j]) > fabs(A[p][j])) p = i;
      if (p != j) {
        for (int k = 0; k < 4; ++k) {
          const double tmp = A[j][k];
          A[j][k] = A[p][k];
          A[p][k] = tmp;
        }
        const int tp = perm[j];
        perm[j] = perm[p];
        perm[p] = tp;
      }
      const double rp = 1.0 / A[j][j];
      for (int i = j + 1; i < 4; ++i) {
        A[i][j] *= rp;
        for (int k = j + 1; k < 4; ++k) A[i][k] -= A[i][j] * A[j][k];
      }
    }
    double x[4];
    for (int i = 0; i < 4; ++i) x[i] = y[perm[i]];
    for (int j = 0; j < 4; ++j)
      for (int i = j + 1; i < 4; ++i) x[i] -= x[j] * A[i][j];
    for (int j = 3; j >= 0; --j) {
      x[j] /= A[j][j];
      for (int i = 0; i < j; ++i) x[i] -= x[j] * A[i][j];
    }
    o.delta = x[2];
    o.gamma = 2.0 * x[1];
  }
  return o;
}

// one thread per trade; the combinations keep the reference's operation
// order (Python evaluation order), so with the same value vectors they are
// bit-identical to the host epilogues of the facades
__global__ void greeks_kernel(int T, const int32_t* __restrict__ tkind,
                              const int32_t* __restrict__ tfirst,
                              const double* __restrict__ tpar, const uint64_t* __restrict__ raddr,
                              const int32_t* __restrict__ rint, const double* __restrict__ rdbl,
                              double* __restrict__ out) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const double* P = tpar + (size_t)t * FDCN_GK_NPARAM;
  const int r0 = tfirst[t];
  auto rd = [&](int k) {
    const int r = r0 + k;
    return read_grid(reinterpret_cast<const double*>(raddr[r]), rint + (size_t)r * FDCN_GK_NRINT,
                     rdbl + (size_t)r * FDCN_GK_NRDBL);
  };
  double* o = out + (size_t)t * FDCN_GK_NOUT;
  double price = 0.0, delta = 0.0, gamma = 0.0, vega = 0.0, theta = 0.0, aux = 0.0;
  const int kind = tkind[t];
  if (kind == FDCN_GK_BARRIER) {
    // _pde_price_and_greeks3 (discrete_barrier_fdm_pricer.py:883-904)
    // P = sigma, spot, carry, div_yield, r, dv
    const Readout b = rd(0), u = rd(1);
    price = b.price;
    delta = b.delta;
    gamma = b.gamma;
    vega = (u.price - b.price) / (P[5] * 100);
    theta = -(0.5 * P[0] * P[0] * P[1] * P[1] * gamma + (P[2] - P[3]) * P[1] * delta -
              P[4] * price);
  } else if (kind == FDCN_GK_CNLOG) {
    // _pde_price_and_greeks (discrete_barrier_fdm_pricer_cn.py:429-466)
    // P = sigma, S0, b, r, dv
    const Readout b = rd(0), u = rd(1), d = rd(2);
    price = b.price;
    delta = b.delta;
    gamma = b.gamma;
    theta = -(0.5 * P[0] * P[0] * P[1] * P[1] * gamma + P[2] * P[1] * delta - P[3] * price);
    vega = (u.price - d.price) / (2.0 * P[4]);
  } else if (kind == FDCN_GK_AMERICAN) {
    // greeks_log2 with Richardson (fd_american_equity.py:970-1068) and the
    // price_log2 Richardson N / 2*num_space_nodes (:925-951) in aux
    // P = sigma, spot, carry, r, h
    const Readout n1 = rd(0), n2 = rd(1);
    price = (4.0 * n2.price - n1.price) / 3.0;
    delta = (4.0 * n2.delta - n1.delta) / 3.0;
    gamma = (4.0 * n2.gamma - n1.gamma) / 3.0;
    const double h = P[4];
    const double first_h = (rd(2).price - rd(3).price) / (2.0 * h);
    const double first_2h = (rd(4).price - rd(5).price) / (4.0 * h);
    const double dvds = (4.0 * first_h - first_2h) / 3.0;
    vega = dvds / 100.0;
    const double q = 0.0;
    theta = -(0.5 * P[0] * P[0] * P[1] * P[1] * gamma + (P[2] - q) * P[1] * delta - P[3] * price);
    aux = (4.0 * rd(6).price - n1.price) / 3.0;
  } else {  // FDCN_GK_READOUT
    const Readout b = rd(0);
    price = b.price;
    delta = b.delta;
    gamma = b.gamma;
  }
  o[0] = price;
  o[1] = delta;
  o[2] = gamma;
  o[3] = vega;
  o[4] = theta;
  o[5] = aux;
}

int readouts_per_kind(int kind) {
  switch (kind) {
    case FDCN_GK_BARRIER: return 2;
    case FDCN_GK_CNLOG: return 3;
    case FDCN_GK_AMERICAN: return 7;
    case FDCN_GK_READOUT: return 1;
    default: return -1;
  }
}

// Pinned staging (fdcn_session_book.h): within a session every async copy
// reads/writes a region no later call of that session reuses; the regions
// are recycled only after fdcn_session_destroy has synchronised the
// session's streams.
struct HipPinned {
  static void* alloc(size_t n) {
    void* p = nullptr;
    return hipHostMalloc(&p, n, hipHostMallocDefault) == hipSuccess ? p : nullptr;
  }
  static void release(void* p) { (void)hipHostFree(p); }
};
using PinnedArena = fdcn_book::PinnedArenaT<HipPinned>;
// pinned staging an idle per-thread context keeps between sessions: enough
// for a whole-file plan (a 10 000-row barrier file stages 131 MB, a 2 000-row
// American file ~400 MB), so repeated files reuse it (pinning it again costs
// ~15-40 ms per file: 34 -> 52 ms per 10 000-row file with a 64 MB cap),
// while the process's locked memory stays bounded per thread
constexpr size_t kIdlePinnedBytes = size_t(1) << 30;

// Per-thread, per-device resources a session borrows: streams, spare events
// and the pinned arena.  Creating them costs far more than a small trade's
// march (streams ~100 us, an 8 MB pinned chunk ~1 ms), so fdcn_session_destroy
// hands them back to the thread's idle list instead of releasing them
// (they live until the process ends).
struct Ctx {
  int device = 0;
  std::vector<hipStream_t> streams;
  std::vector<hipEvent_t> spare_events;
  PinnedArena pinned;
};
thread_local std::vector<Ctx*> t_idle_ctx;

}  // namespace

struct fdcn_session {
  int device = 0;
  Ctx* ctx = nullptr;
  std::vector<hipStream_t> streams;  // the ctx streams this session has used
  int rr = 0;
  std::vector<hipEvent_t> events;
  fdcn_book::SlotTable slots;
  fdcn_book::RegionTable regions;
  struct Block {
    void* p;
    hipStream_t s;
  };
  std::vector<Block> blocks;
  PinnedArena& pinned() { return ctx->pinned; }
};

namespace {

int pick_stream(fdcn_session* s, hipStream_t* out) {
  if ((int)s->streams.size() < kMaxStreams) {
    Ctx* c = s->ctx;
    if (c->streams.size() <= s->streams.size()) {
      hipStream_t st;
      S_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
      c->streams.push_back(st);
    }
    hipStream_t st = c->streams[s->streams.size()];
    s->streams.push_back(st);
    *out = st;
    return FDCN_OK;
  }
  *out = s->streams[s->rr++ % kMaxStreams];
  return FDCN_OK;
}

int check_slots(fdcn_session* s, int32_t n, const int32_t* slots, int32_t n_nodes) {
  char err[160];
  if (s->slots.check(n, slots, n_nodes, err, sizeof(err))) return sfail(FDCN_EINVAL, "%s", err);
  return FDCN_OK;
}

// make `st` wait for the launches that produced the given slots
int wait_producers(fdcn_session* s, hipStream_t st, int32_t n, const int32_t* slots) {
  for (int32_t e : s->slots.producers(n, slots)) S_TRY(hipStreamWaitEvent(st, s->events[e], 0));
  return FDCN_OK;
}

int alloc_block(fdcn_session* s, hipStream_t st, size_t bytes, char** out) {
  void* p = nullptr;
  hipError_t e = hipMallocAsync(&p, bytes, st);
  if (e != hipSuccess)
    return sfail(FDCN_ENOMEM, "hipMallocAsync(%zu): %s", bytes, hipGetErrorString(e));
  s->blocks.push_back({p, st});
  *out = (char*)p;
  return FDCN_OK;
}

// record the completion of the work just queued on `st`; returns the event id
int record(fdcn_session* s, hipStream_t st, int32_t* ev) {
  hipEvent_t e;
  if (!s->ctx->spare_events.empty()) {
    e = s->ctx->spare_events.back();
    s->ctx->spare_events.pop_back();
  } else {
    S_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  S_TRY(hipEventRecord(e, st));
  s->events.push_back(e);
  *ev = (int32_t)s->events.size() - 1;
  return FDCN_OK;
}

int new_slots(fdcn_session* s, double* base, int32_t B, int32_t n_nodes, int32_t ev,
              int32_t* out_slots) {
  s->slots.add(base, B, n_nodes, ev, out_slots);
  return FDCN_OK;
}

}  // namespace

extern "C" {

int fdcn_session_create(fdcn_session** out) {
  if (!out) return sfail(FDCN_EINVAL, "fdcn_session_create: NULL out");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    return sfail(FDCN_ENODEV, "no HIP device visible");
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return sfail(FDCN_EHIP, "hipGetDevice failed");
  Ctx* c = nullptr;
  for (size_t i = 0; i < t_idle_ctx.size(); ++i)
    if (t_idle_ctx[i]->device == dev) {
      c = t_idle_ctx[i];
      t_idle_ctx.erase(t_idle_ctx.begin() + (long)i);
      break;
    }
  if (!c) {
    c = new Ctx();
    c->device = dev;
    hipMemPool_t pool;
    if (hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess) {
      uint64_t keep = UINT64_MAX;  // keep freed blocks in the pool between sessions
      (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
  }
  fdcn_session* s = new fdcn_session();
  s->device = dev;
  s->ctx = c;
  *out = s;
  return FDCN_OK;
}

int fdcn_session_destroy(fdcn_session* s) {
  if (!s) return FDCN_OK;
  int rc = FDCN_OK;
  int cur = 0;
  (void)hipGetDevice(&cur);
  if (cur != s->device) (void)hipSetDevice(s->device);
  // Drain every session stream BEFORE the frees: a block allocated on one
  // stream is read on others (gather_rows of v_init slots, the dividend
  // jump, the Greeks epilogue wait on its producer's event), so a free
  // ordered on the allocating stream alone could hand the block to another
  // allocation while a consumer still reads it.  After the syncs no work of
  // the session is pending and the stream-ordered frees are safe.
  for (hipStream_t st : s->streams)
    if (hipStreamSynchronize(st) != hipSuccess) rc = sfail(FDCN_EHIP, "stream sync failed");
  if (rc == FDCN_OK) {
    for (auto& b : s->blocks)
      if (hipFreeAsync(b.p, b.s) != hipSuccess) rc = sfail(FDCN_EHIP, "hipFreeAsync failed");
  }  // after a failure the blocks are leaked rather than freed under running work
  if (rc == FDCN_OK) {  // everything drained: the resources go back to the thread
    for (hipEvent_t e : s->events) s->ctx->spare_events.push_back(e);
    s->ctx->pinned.reset();
    s->ctx->pinned.trim(kIdlePinnedBytes);
    t_idle_ctx.push_back(s->ctx);
  }  // after a failure they are dropped (leaked) rather than reused
  if (cur != s->device) (void)hipSetDevice(cur);
  delete s;
  return rc;
}

int fdcn_session_slots(const fdcn_session* s) { return s ? (int)s->slots.size() : -1; }

int fdcn_session_host_buffer(fdcn_session* s, int64_t bytes, void** out) {
  if (!s || !out || bytes < 0) return sfail(FDCN_EINVAL, "fdcn_session_host_buffer: bad argument");
  *out = s->pinned().get((size_t)bytes);
  if (!*out) return sfail(FDCN_ENOMEM, "hipHostMalloc(%lld) failed", (long long)bytes);
  return FDCN_OK;
}

// fdcn_session_march and fdcn_session_march_ps: the IT payoff is the host
// array `payoff` or the vectors in `payoff_slots` (at most one of them)
static int session_march(fdcn_session* s, int32_t it, int32_t B, int32_t n_nodes, int32_t n_time,
                         int32_t n_ranna, const double* params, const int32_t* iparams,
                         const double* v_init, const int32_t* v_init_slots,
                         const double* payoff, const int32_t* payoff_slots, int32_t n_mon,
                         const int32_t* mon_step, const double* mon_rebate, int32_t* out_slots) {
  if (!s) return sfail(FDCN_EINVAL, "NULL session");
  it = it ? 1 : 0;
  int rc = fdcn_internal::validate_plan(it, B, n_nodes, n_time, n_ranna, params, iparams, n_mon,
                                        mon_step, mon_rebate);
  if (rc) return rc;
  if (B == 0) return FDCN_OK;
  if (!out_slots) return sfail(FDCN_EINVAL, "NULL out_slots");
  if ((v_init == nullptr) == (v_init_slots == nullptr))
    return sfail(FDCN_EINVAL, "pass exactly one of v_init (host) and v_init_slots");
  if (it && !payoff && !payoff_slots) return sfail(FDCN_EINVAL, "IT march without payoff");
  if (v_init_slots && (rc = check_slots(s, B, v_init_slots, n_nodes))) return rc;
  if (payoff_slots && (rc = check_slots(s, B, payoff_slots, n_nodes))) return rc;
  // payoff slots that are consecutive vectors of one block (one upload) are
  // the [B][n_nodes] array the march reads; any other set is gathered into one
  bool ps_gather = false;
  for (int32_t b = 1; payoff_slots && b < B; ++b)
    if ((uint64_t)s->slots.ptr[payoff_slots[b]] !=
        (uint64_t)s->slots.ptr[payoff_slots[0]] + sizeof(double) * (uint64_t)b * n_nodes)
      ps_gather = true;
  const int k_cap = fdcn_sm_extent(B, n_nodes, n_time, n_ranna, params);
  if (k_cap < 0) return k_cap;
  int32_t w_, npt_, spb_, lds_;
  int64_t ws_ = 0;
  if ((rc = fdcn_plan(B, n_nodes, n_time, it, k_cap, &w_, &npt_, &spb_, &lds_, &ws_))) return rc;

  const size_t nv = (size_t)B * n_nodes, nm = (size_t)(n_mon > 0 ? n_mon : 1);
  const size_t vb = sizeof(double) * nv;
  // the small inputs, the payoff and v_init, then device-only buffers
  Layout L;
  const size_t oP = L.add(sizeof(double) * B * FDCN_NPARAM);
  const size_t oI = L.add(sizeof(int32_t) * B * FDCN_NIPARAM);
  const size_t oM = L.add(sizeof(int32_t) * nm);
  const size_t oR = L.add(sizeof(double) * nm);
  const size_t oA = v_init_slots ? L.add(sizeof(uint64_t) * B) : 0;
  const size_t oAF = ps_gather ? L.add(sizeof(uint64_t) * B) : 0;
  const size_t pre = L.size;  // the small inputs: [0, pre)
  const size_t oF = it && (!payoff_slots || ps_gather) ? L.add(vb) : 0;
  // an IT march whose host v_init is its payoff array (the first segment of
  // an American grid) copies that array once and reads it twice
  const bool v_is_payoff = it && v_init && v_init == payoff;
  const size_t oV = L.add(vb);  // copied only for a host v_init
  const size_t oO = L.add(vb);
  const size_t ws_bytes = (size_t)ws_ * (size_t)B;
  const size_t oW = L.add(ws_bytes);
  // A payoff / v_init inside this session's pinned memory (from
  // fdcn_session_host_buffer: a plan written straight into it) is copied to
  // the device from where it lies; anything else is staged.  The staging
  // block mirrors the device offsets up to the first array copied directly,
  // so the common all-staged case is one H2D copy.
  const bool f_host = it && !payoff_slots;
  const bool f_direct = f_host && s->pinned().owns(payoff, vb);
  const bool v_host = v_init && !v_is_payoff;
  const bool v_direct = v_host && s->pinned().owns(v_init, vb);
  const bool stage_f = f_host && !f_direct, stage_v = v_host && !v_direct;
  size_t hsz = pre, hF = 0, hV = 0;
  if (stage_f) hF = hsz, hsz = oF + al256(vb);
  if (stage_v) hV = it ? (stage_f ? oV : pre) : oV, hsz = hV + al256(vb);
  const size_t mirrored = stage_v && hV == oV ? oV + vb : stage_f ? oF + vb : pre;

  char* h = s->pinned().get(hsz);
  if (!h) return sfail(FDCN_ENOMEM, "hipHostMalloc(%zu) failed", hsz);
  memcpy(h + oP, params, sizeof(double) * B * FDCN_NPARAM);
  memcpy(h + oI, iparams, sizeof(int32_t) * B * FDCN_NIPARAM);
  if (n_mon > 0) {
    memcpy(h + oM, mon_step, sizeof(int32_t) * n_mon);
    memcpy(h + oR, mon_rebate, sizeof(double) * n_mon);
  }
  if (v_init_slots) {
    uint64_t* a = (uint64_t*)(h + oA);
    for (int32_t b = 0; b < B; ++b) a[b] = (uint64_t)s->slots.ptr[v_init_slots[b]];
  }
  if (ps_gather) {
    uint64_t* a = (uint64_t*)(h + oAF);
    for (int32_t b = 0; b < B; ++b) a[b] = (uint64_t)s->slots.ptr[payoff_slots[b]];
  }
  if (stage_f) stage_copy(h + hF, payoff, vb);
  if (stage_v) stage_copy(h + hV, v_init, vb);
  hipStream_t st;
  if ((rc = pick_stream(s, &st))) return rc;
  if (v_init_slots && (rc = wait_producers(s, st, B, v_init_slots))) return rc;
  if (payoff_slots && (rc = wait_producers(s, st, B, payoff_slots))) return rc;
  char* d = nullptr;
  if ((rc = alloc_block(s, st, L.size, &d))) return rc;
  S_TRY(hipMemcpyAsync(d, h, mirrored, hipMemcpyHostToDevice, st));
  if (f_direct) S_TRY(hipMemcpyAsync(d + oF, payoff, vb, hipMemcpyHostToDevice, st));
  if (stage_v && hV != oV) S_TRY(hipMemcpyAsync(d + oV, h + hV, vb, hipMemcpyHostToDevice, st));
  if (v_direct) S_TRY(hipMemcpyAsync(d + oV, v_init, vb, hipMemcpyHostToDevice, st));
  if (v_init_slots) {
    hipLaunchKernelGGL(gather_rows, dim3(B), dim3(256), 0, st, (const uint64_t*)(d + oA),
                       (double*)(d + oV), n_nodes);
    S_TRY(hipGetLastError());
  }
  if (ps_gather) {
    hipLaunchKernelGGL(gather_rows, dim3(B), dim3(256), 0, st, (const uint64_t*)(d + oAF),
                       (double*)(d + oF), n_nodes);
    S_TRY(hipGetLastError());
  }
  const double* d_payoff = payoff_slots && !ps_gather ? s->slots.ptr[payoff_slots[0]]
                                                      : (const double*)(d + oF);
  rc = fdcn_internal::launch_march(it, B, n_nodes, n_time, n_ranna, (const double*)(d + oP),
                                   (const int32_t*)(d + oI),
                                   (const double*)(d + (v_is_payoff ? oF : oV)),
                                   it ? d_payoff : nullptr, n_mon,
                                   (const int32_t*)(d + oM), (const double*)(d + oR),
                                   (double*)(d + oO), k_cap, (double*)(d + oW),
                                   (int64_t)ws_bytes, st);
  if (rc) return rc;
  int32_t ev;
  if ((rc = record(s, st, &ev))) return rc;
  return new_slots(s, (double*)(d + oO), B, n_nodes, ev, out_slots);
}

int fdcn_session_march(fdcn_session* s, int32_t it, int32_t B, int32_t n_nodes, int32_t n_time,
                       int32_t n_ranna, const double* params, const int32_t* iparams,
                       const double* v_init, const int32_t* v_init_slots, const double* payoff,
                       int32_t n_mon, const int32_t* mon_step, const double* mon_rebate,
                       int32_t* out_slots) {
  return session_march(s, it, B, n_nodes, n_time, n_ranna, params, iparams, v_init, v_init_slots,
                       payoff, nullptr, n_mon, mon_step, mon_rebate, out_slots);
}

int fdcn_session_march_ps(fdcn_session* s, int32_t it, int32_t B, int32_t n_nodes,
                          int32_t n_time, int32_t n_ranna, const double* params,
                          const int32_t* iparams, const double* v_init,
                          const int32_t* v_init_slots, const int32_t* payoff_slots,
                          int32_t n_mon, const int32_t* mon_step, const double* mon_rebate,
                          int32_t* out_slots) {
  if (B < 1 || n_nodes < 1) return sfail(FDCN_EINVAL, "march_ps: B >= 1, n_nodes >= 1");
  if (!it) return sfail(FDCN_EINVAL, "march_ps: payoff slots belong to an IT march (it != 0)");
  if (!payoff_slots) return sfail(FDCN_EINVAL, "march_ps: NULL payoff_slots");
  return session_march(s, it, B, n_nodes, n_time, n_ranna, params, iparams, v_init, v_init_slots,
                       nullptr, payoff_slots, n_mon, mon_step, mon_rebate, out_slots);
}

int fdcn_session_upload(fdcn_session* s, int32_t B, int32_t n_nodes, const double* v,
                        int32_t* out_slots) {
  if (B < 1 || n_nodes < 1) return sfail(FDCN_EINVAL, "upload: B >= 1, n_nodes >= 1");
  if (!v || !out_slots) return sfail(FDCN_EINVAL, "upload: NULL argument");
  if (!s) return sfail(FDCN_EINVAL, "NULL session");
  const size_t vb = sizeof(double) * (size_t)B * n_nodes;
  const void* src = v;  // inside the session's pinned memory: read where it lies
  if (!s->pinned().owns(v, vb)) {
    char* h = s->pinned().get(vb);
    if (!h) return sfail(FDCN_ENOMEM, "hipHostMalloc(%zu) failed", vb);
    stage_copy(h, v, vb);
    src = h;
  }
  hipStream_t st;
  int rc = pick_stream(s, &st);
  if (rc) return rc;
  char* d = nullptr;
  if ((rc = alloc_block(s, st, vb, &d))) return rc;
  S_TRY(hipMemcpyAsync(d, src, vb, hipMemcpyHostToDevice, st));
  int32_t ev;
  if ((rc = record(s, st, &ev))) return rc;
  return new_slots(s, (double*)d, B, n_nodes, ev, out_slots);
}

int fdcn_session_knockout(fdcn_session* s, int32_t B, int32_t n_nodes, const int32_t* slots,
                          const int32_t* ko_lo, const int32_t* ko_hi, const double* rebate,
                          const int32_t* floor_slots) {
  if (B < 1 || n_nodes < 1) return sfail(FDCN_EINVAL, "knockout: B >= 1, n_nodes >= 1");
  if (!slots || !ko_lo || !ko_hi || !rebate)
    return sfail(FDCN_EINVAL, "knockout: NULL argument (slots, ko_lo, ko_hi, rebate)");
  if (!s) return sfail(FDCN_EINVAL, "NULL session");
  const int64_t chunks = ((int64_t)n_nodes + 255) / 256;
  if (chunks * B > INT32_MAX) return sfail(FDCN_EINVAL, "knockout: batch too large for one launch");
  int rc = check_slots(s, B, slots, n_nodes);
  if (rc) return rc;
  if (floor_slots && (rc = check_slots(s, B, floor_slots, n_nodes))) return rc;
  // the event writes in place: a slot named twice, or read as a floor while
  // another vector's event writes it, would make the result depend on timing
  std::vector<int32_t> sorted(slots, slots + B);
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
    return sfail(FDCN_EINVAL, "knockout: a slot appears twice in slots");
  for (int32_t b = 0; floor_slots && b < B; ++b)
    if (std::binary_search(sorted.begin(), sorted.end(), floor_slots[b]))
      return sfail(FDCN_EINVAL, "knockout: floor slot %d is one of slots", floor_slots[b]);
  Layout L;
  const size_t oA = L.add(sizeof(uint64_t) * B);
  const size_t oF = L.add(sizeof(uint64_t) * B);
  const size_t oLo = L.add(sizeof(int32_t) * B);
  const size_t oHi = L.add(sizeof(int32_t) * B);
  const size_t oR = L.add(sizeof(double) * B);
  char* h = s->pinned().get(L.size);
  if (!h) return sfail(FDCN_ENOMEM, "hipHostMalloc(%zu) failed", L.size);
  uint64_t* a = (uint64_t*)(h + oA);
  uint64_t* f = (uint64_t*)(h + oF);
  for (int32_t b = 0; b < B; ++b) {
    a[b] = (uint64_t)s->slots.ptr[slots[b]];
    f[b] = floor_slots ? (uint64_t)s->slots.ptr[floor_slots[b]] : 0;
  }
  memcpy(h + oLo, ko_lo, sizeof(int32_t) * B);
  memcpy(h + oHi, ko_hi, sizeof(int32_t) * B);
  memcpy(h + oR, rebate, sizeof(double) * B);
  hipStream_t st;
  if ((rc = pick_stream(s, &st))) return rc;
  // In place: the event runs after everything the session has queued so far,
  // on every stream -- the march that produced the slots (and the upload of
  // the floor), and any earlier call that still reads them.  Deliberately
  // conservative: one fresh event per other stream (up to 3 a call, kept
  // until destroy) instead of the slots' producer events plus a per-slot
  // "last reader", which the slot table does not keep.  It joins the
  // session's streams at every monitoring date, so launch groups of
  // different shapes overlap within a segment round but not across one.
  for (hipStream_t other : s->streams) {
    if (other == st) continue;
    int32_t ev;
    if ((rc = record(s, other, &ev))) return rc;
    S_TRY(hipStreamWaitEvent(st, s->events[ev], 0));
  }
  char* d = nullptr;
  if ((rc = alloc_block(s, st, L.size, &d))) return rc;
  S_TRY(hipMemcpyAsync(d, h, L.size, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(knockout_kernel, dim3((unsigned)(chunks * B)), dim3(256), 0, st, n_nodes,
                     (int)chunks, (const uint64_t*)(d + oA),
                     floor_slots ? (const uint64_t*)(d + oF) : nullptr,
                     (const int32_t*)(d + oLo), (const int32_t*)(d + oHi),
                     (const double*)(d + oR));
  S_TRY(hipGetLastError());
  int32_t ev;
  if ((rc = record(s, st, &ev))) return rc;
  for (int32_t b = 0; b < B; ++b) s->slots.ev[(size_t)slots[b]] = ev;  // consumers wait for it
  return FDCN_OK;
}

int fdcn_session_knockin(fdcn_session* s, int32_t B, int32_t n_nodes, const int32_t* slots,
                         const int32_t* src_slots, const int32_t* ko_lo, const int32_t* ko_hi) {
  if (B < 1 || n_nodes < 1) return sfail(FDCN_EINVAL, "knockin: B >= 1, n_nodes >= 1");
  if (!slots || !src_slots || !ko_lo || !ko_hi)
    return sfail(FDCN_EINVAL, "knockin: NULL argument (slots, src_slots, ko_lo, ko_hi)");
  if (!s) return sfail(FDCN_EINVAL, "NULL session");
  const int64_t chunks = ((int64_t)n_nodes + 255) / 256;
  if (chunks * B > INT32_MAX) return sfail(FDCN_EINVAL, "knockin: batch too large for one launch");
  int rc = check_slots(s, B, slots, n_nodes);
  if (rc) return rc;
  if ((rc = check_slots(s, B, src_slots, n_nodes))) return rc;
  // as the knock-out: in place, so a slot named twice, or read as a source
  // while another vector's event writes it, would depend on timing
  std::vector<int32_t> sorted(slots, slots + B);
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
    return sfail(FDCN_EINVAL, "knockin: a slot appears twice in slots");
  for (int32_t b = 0; b < B; ++b)
    if (std::binary_search(sorted.begin(), sorted.end(), src_slots[b]))
      return sfail(FDCN_EINVAL, "knockin: source slot %d is one of slots", src_slots[b]);
  Layout L;
  const size_t oA = L.add(sizeof(uint64_t) * B);
  const size_t oS = L.add(sizeof(uint64_t) * B);
  const size_t oLo = L.add(sizeof(int32_t) * B);
  const size_t oHi = L.add(sizeof(int32_t) * B);
  char* h = s->pinned().get(L.size);
  if (!h) return sfail(FDCN_ENOMEM, "hipHostMalloc(%zu) failed", L.size);
  uint64_t* a = (uint64_t*)(h + oA);
  uint64_t* f = (uint64_t*)(h + oS);
  for (int32_t b = 0; b < B; ++b) {
    a[b] = (uint64_t)s->slots.ptr[slots[b]];
    f[b] = (uint64_t)s->slots.ptr[src_slots[b]];
  }
  memcpy(h + oLo, ko_lo, sizeof(int32_t) * B);
  memcpy(h + oHi, ko_hi, sizeof(int32_t) * B);
  hipStream_t st;
  if ((rc = pick_stream(s, &st))) return rc;
  // The ordering of fdcn_session_knockout: after everything the session has
  // queued so far on every stream, which covers the marches that produced
  // `slots` and the sources (often on another stream: the IT and the CN chain
  // are different launch groups) and any earlier reader of `slots`.
  for (hipStream_t other : s->streams) {
    if (other == st) continue;
    int32_t ev;
    if ((rc = record(s, other, &ev))) return rc;
    S_TRY(hipStreamWaitEvent(st, s->events[ev], 0));
  }
  char* d = nullptr;
  if ((rc = alloc_block(s, st, L.size, &d))) return rc;
  S_TRY(hipMemcpyAsync(d, h, L.size, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(knockin_kernel, dim3((unsigned)(chunks * B)), dim3(256), 0, st, n_nodes,
                     (int)chunks, (const uint64_t*)(d + oA), (const uint64_t*)(d + oS),
                     (const int32_t*)(d + oLo), (const int32_t*)(d + oHi));
  S_TRY(hipGetLastError());
  int32_t ev;
  if ((rc = record(s, st, &ev))) return rc;
  for (int32_t b = 0; b < B; ++b) s->slots.ev[(size_t)slots[b]] = ev;  // consumers wait for it
  return FDCN_OK;
}

int fdcn_session_exercise(fdcn_session* s, int32_t B, int32_t n_nodes, const int32_t* slots,
                          const int32_t* floor_slots, const int32_t* ko_lo, const int32_t* ko_hi,
                          const double* rebate, int32_t* out_region_ids) {
  if (B < 1 || n_nodes < 1) return sfail(FDCN_EINVAL, "exercise: B >= 1, n_nodes >= 1");
  if (!slots || !floor_slots || !out_region_ids)
    return sfail(FDCN_EINVAL, "exercise: NULL argument (slots, floor_slots, out_region_ids)");
  const bool barrier = ko_lo || ko_hi || rebate;
  if (barrier && !(ko_lo && ko_hi && rebate))
    return sfail(FDCN_EINVAL, "exercise: ko_lo, ko_hi and rebate go together (all or none)");
  if (!s) return sfail(FDCN_EINVAL, "NULL session");
  int rc = check_slots(s, B, slots, n_nodes);
  if (rc) return rc;
  if ((rc = check_slots(s, B, floor_slots, n_nodes))) return rc;
  // as the knock-out: in place, so a slot named twice, or read as a floor
  // while another vector's event writes it, would depend on timing
  std::vector<int32_t> sorted(slots, slots + B);
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
    return sfail(FDCN_EINVAL, "exercise: a slot appears twice in slots");
  for (int32_t b = 0; b < B; ++b)
    if (std::binary_search(sorted.begin(), sorted.end(), floor_slots[b]))
      return sfail(FDCN_EINVAL, "exercise: floor slot %d is one of slots", floor_slots[b]);
  Layout L;
  const size_t oA = L.add(sizeof(uint64_t) * B);
  const size_t oF = L.add(sizeof(uint64_t) * B);
  const size_t oLo = L.add(sizeof(int32_t) * B);
  const size_t oHi = L.add(sizeof(int32_t) * B);
  const size_t oR = L.add(sizeof(double) * B);
  const size_t in_bytes = L.size;
  const size_t oG = L.add(sizeof(int32_t) * 3 * (size_t)B);  // the region records (device only)
  char* h = s->pinned().get(in_bytes);
  if (!h) return sfail(FDCN_ENOMEM, "hipHostMalloc(%zu) failed", in_bytes);
  uint64_t* a = (uint64_t*)(h + oA);
  uint64_t* f = (uint64_t*)(h + oF);
  for (int32_t b = 0; b < B; ++b) {
    a[b] = (uint64_t)s->slots.ptr[slots[b]];
    f[b] = (uint64_t)s->slots.ptr[floor_slots[b]];
  }
  if (barrier) {
    memcpy(h + oLo, ko_lo, sizeof(int32_t) * B);
    memcpy(h + oHi, ko_hi, sizeof(int32_t) * B);
    memcpy(h + oR, rebate, sizeof(double) * B);
  }
  hipStream_t st;
  if ((rc = pick_stream(s, &st))) return rc;
  // The ordering of fdcn_session_knockout: after everything the session has
  // queued so far on every stream (the march that produced the slots, the
  // upload of the floor, any earlier reader of the slots).
  for (hipStream_t other : s->streams) {
    if (other == st) continue;
    int32_t ev;
    if ((rc = record(s, other, &ev))) return rc;
    S_TRY(hipStreamWaitEvent(st, s->events[ev], 0));
  }
  char* d = nullptr;
  if ((rc = alloc_block(s, st, L.size, &d))) return rc;
  S_TRY(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(exercise_kernel, dim3((unsigned)B), dim3(256), 0, st, n_nodes,
                     (const uint64_t*)(d + oA), (const uint64_t*)(d + oF),
                     barrier ? (const int32_t*)(d + oLo) : nullptr,
                     barrier ? (const int32_t*)(d + oHi) : nullptr,
                     barrier ? (const double*)(d + oR) : nullptr, (int32_t*)(d + oG));
  S_TRY(hipGetLastError());
  int32_t ev;
  if ((rc = record(s, st, &ev))) return rc;
  for (int32_t b = 0; b < B; ++b) s->slots.ev[(size_t)slots[b]] = ev;  // consumers wait for it
  s->regions.add((int32_t*)(d + oG), B, ev, out_region_ids);
  return FDCN_OK;
}

int fdcn_session_exercise_regions(fdcn_session* s, int32_t n, const int32_t* ids, int32_t* out) {
  if (!s) return sfail(FDCN_EINVAL, "NULL session");
  if (n < 0) return sfail(FDCN_EINVAL, "exercise_regions: n >= 0");
  if (n == 0) return FDCN_OK;
  if (!ids || !out) return sfail(FDCN_EINVAL, "exercise_regions: NULL argument");
  char err[160];
  if (s->regions.check(n, ids, err, sizeof(err))) return sfail(FDCN_EINVAL, "%s", err);
  const size_t rec = sizeof(int32_t) * 3;
  char* h = s->pinned().get(rec * (size_t)n);
  if (!h) return sfail(FDCN_ENOMEM, "hipHostMalloc(%zu) failed", rec * (size_t)n);
  hipStream_t st;
  int rc = pick_stream(s, &st);
  if (rc) return rc;
  for (int32_t e : s->regions.producers(n, ids)) S_TRY(hipStreamWaitEvent(st, s->events[e], 0));
  // consecutive ids of one call are consecutive records: one copy per run
  for (int32_t i = 0; i < n;) {
    int32_t k = i + 1;
    while (k < n && s->regions.ev[(size_t)ids[k]] == s->regions.ev[(size_t)ids[k - 1]] &&
           s->regions.ptr[(size_t)ids[k]] == s->regions.ptr[(size_t)ids[k - 1]] + 3)
      ++k;
    S_TRY(hipMemcpyAsync(h + rec * (size_t)i, s->regions.ptr[(size_t)ids[i]], rec * (size_t)(k - i),
                         hipMemcpyDeviceToHost, st));
    i = k;
  }
  S_TRY(hipStreamSynchronize(st));
  memcpy(out, h, rec * (size_t)n);
  return FDCN_OK;
}

int fdcn_session_dividend_jump(fdcn_session* s, int32_t B, int32_t n_nodes,
                               const int32_t* in_slots, const double* s_nodes,
                               const double* cash_div, const double* strike_call,
                               int32_t* out_slots) {
  if (!s) return sfail(FDCN_EINVAL, "NULL session");
  if (B < 0 || n_nodes < 2) return sfail(FDCN_EINVAL, "dividend jump: B >= 0, n_nodes >= 2");
  if (B == 0) return FDCN_OK;
  if (!in_slots || !s_nodes || !cash_div || !strike_call || !out_slots)
    return sfail(FDCN_EINVAL, "dividend jump: NULL argument");
  int rc = check_slots(s, B, in_slots, n_nodes);
  if (rc) return rc;
  for (int32_t b = 0; b < B; ++b)
    for (int32_t i = 0; i + 1 < n_nodes; ++i)
      if (!(s_nodes[(size_t)b * n_nodes + i + 1] - s_nodes[(size_t)b * n_nodes + i] > 0.0))
        return sfail(FDCN_EINVAL, "x must be strictly increasing.");
  const size_t nv = (size_t)B * n_nodes;
  Layout L;
  const size_t oA = L.add(sizeof(uint64_t) * B);
  const size_t oS = L.add(sizeof(double) * nv);
  const size_t oC = L.add(sizeof(double) * B);
  const size_t oK = L.add(sizeof(double) * B);
  const size_t staged = L.size;
  const size_t oO = L.add(sizeof(double) * nv);
  const size_t oW = L.add(sizeof(double) * 3 * nv);
  char* h = s->pinned().get(staged);
  if (!h) return sfail(FDCN_ENOMEM, "hipHostMalloc(%zu) failed", staged);
  uint64_t* a = (uint64_t*)(h + oA);
  for (int32_t b = 0; b < B; ++b) a[b] = (uint64_t)s->slots.ptr[in_slots[b]];
  stage_copy(h + oS, s_nodes, sizeof(double) * nv);
  memcpy(h + oC, cash_div, sizeof(double) * B);
  memcpy(h + oK, strike_call, sizeof(double) * B);
  hipStream_t st;
  if ((rc = pick_stream(s, &st))) return rc;
  if ((rc = wait_producers(s, st, B, in_slots))) return rc;
  char* d = nullptr;
  if ((rc = alloc_block(s, st, L.size, &d))) return rc;
  S_TRY(hipMemcpyAsync(d, h, staged, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(dividend_jump_kernel, dim3(B), dim3(64), 0, st, n_nodes,
                     (const uint64_t*)(d + oA), (const double*)(d + oS), (const double*)(d + oC),
                     (const double*)(d + oK), (double*)(d + oO), (double*)(d + oW));
  S_TRY(hipGetLastError());
  int32_t ev;
  if ((rc = record(s, st, &ev))) return rc;
  return new_slots(s, (double*)(d + oO), B, n_nodes, ev, out_slots);
}

int fdcn_session_greeks(fdcn_session* s, int32_t T, const int32_t* kind, const int32_t* first,
                        const double* tparams, int32_t R, const int32_t* rint,
                        const double* rdbl, double* out) {
  if (!s) return sfail(FDCN_EINVAL, "NULL session");
  if (T < 0 || R < 0) return sfail(FDCN_EINVAL, "greeks: T, R >= 0");
  if (T == 0) return FDCN_OK;
  if (!kind || !first || !tparams || !rint || !rdbl || !out)
    return sfail(FDCN_EINVAL, "greeks: NULL argument");
  for (int32_t t = 0; t < T; ++t) {
    const int k = readouts_per_kind(kind[t]);
    if (k < 0) return sfail(FDCN_EINVAL, "trade %d: unknown kind %d", t, kind[t]);
    if (first[t] < 0 || first[t] + k > R)
      return sfail(FDCN_EINVAL, "trade %d: readouts [%d,+%d) outside R=%d", t, first[t], k, R);
  }
  std::vector<int32_t> slots(R);
  for (int32_t r = 0; r < R; ++r) {
    const int32_t* ri = rint + (size_t)r * FDCN_GK_NRINT;
    slots[r] = ri[0];
    int rc = check_slots(s, 1, &ri[0], -1);
    if (rc) return rc;
    const int n = s->slots.n[ri[0]];
    const bool ok_i = (ri[1] == 1) || (ri[1] == 2 && ri[2] >= 0 && ri[2] < n) ||
                      (ri[1] == 0 && ri[2] >= 0 && ri[2] + 1 < n);
    const bool ok_d = (ri[4] == 0) || (ri[4] == 1 && ri[3] >= 1 && ri[3] + 1 < n) ||
                      (ri[4] == 2 && ri[3] >= 1 && ri[3] + 2 < n);
    if (!ok_i || !ok_d)
      return sfail(FDCN_EINVAL, "readout %d: node indices outside its %d-node vector", r, n);
  }
  Layout L;
  const size_t oA = L.add(sizeof(uint64_t) * R);
  const size_t oRI = L.add(sizeof(int32_t) * R * FDCN_GK_NRINT);
  const size_t oRD = L.add(sizeof(double) * R * FDCN_GK_NRDBL);
  const size_t oK = L.add(sizeof(int32_t) * T);
  const size_t oF = L.add(sizeof(int32_t) * T);
  const size_t oP = L.add(sizeof(double) * T * FDCN_GK_NPARAM);
  const size_t staged = L.size;
  const size_t oO = L.add(sizeof(double) * T * FDCN_GK_NOUT);
  char* h = s->pinned().get(L.size);
  if (!h) return sfail(FDCN_ENOMEM, "hipHostMalloc(%zu) failed", L.size);
  uint64_t* a = (uint64_t*)(h + oA);
  for (int32_t r = 0; r < R; ++r) a[r] = (uint64_t)s->slots.ptr[slots[r]];
  memcpy(h + oRI, rint, sizeof(int32_t) * R * FDCN_GK_NRINT);
  memcpy(h + oRD, rdbl, sizeof(double) * R * FDCN_GK_NRDBL);
  memcpy(h + oK, kind, sizeof(int32_t) * T);
  memcpy(h + oF, first, sizeof(int32_t) * T);
  memcpy(h + oP, tparams, sizeof(double) * T * FDCN_GK_NPARAM);
  hipStream_t st;
  int rc = pick_stream(s, &st);
  if (rc) return rc;
  if ((rc = wait_producers(s, st, R, slots.data()))) return rc;
  char* d = nullptr;
  if ((rc = alloc_block(s, st, L.size, &d))) return rc;
  S_TRY(hipMemcpyAsync(d, h, staged, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(greeks_kernel, dim3((T + 63) / 64), dim3(64), 0, st, T,
                     (const int32_t*)(d + oK), (const int32_t*)(d + oF),
                     (const double*)(d + oP), (const uint64_t*)(d + oA),
                     (const int32_t*)(d + oRI), (const double*)(d + oRD), (double*)(d + oO));
  S_TRY(hipGetLastError());
  S_TRY(hipMemcpyAsync(h + oO, d + oO, sizeof(double) * T * FDCN_GK_NOUT, hipMemcpyDeviceToHost,
                       st));
  S_TRY(hipStreamSynchronize(st));
  memcpy(out, h + oO, sizeof(double) * T * FDCN_GK_NOUT);
  return FDCN_OK;
}

int fdcn_session_fetch(fdcn_session* s, int32_t n, const int32_t* slots, int32_t n_nodes,
                       double* out) {
  if (!s) return sfail(FDCN_EINVAL, "NULL session");
  if (n < 0 || n_nodes < 1) return sfail(FDCN_EINVAL, "fetch: n >= 0, n_nodes >= 1");
  if (n == 0) return FDCN_OK;
  if (!slots || !out) return sfail(FDCN_EINVAL, "fetch: NULL argument");
  int rc = check_slots(s, n, slots, n_nodes);
  if (rc) return rc;
  const size_t bytes = sizeof(double) * (size_t)n * n_nodes;
  Layout L;
  const size_t oA = L.add(sizeof(uint64_t) * n);
  const size_t oO = L.add(bytes);
  char* h = s->pinned().get(L.size);
  if (!h) return sfail(FDCN_ENOMEM, "hipHostMalloc(%zu) failed", L.size);
  uint64_t* a = (uint64_t*)(h + oA);
  for (int32_t i = 0; i < n; ++i) a[i] = (uint64_t)s->slots.ptr[slots[i]];
  hipStream_t st;
  if ((rc = pick_stream(s, &st))) return rc;
  if ((rc = wait_producers(s, st, n, slots))) return rc;
  char* d = nullptr;
  if ((rc = alloc_block(s, st, L.size, &d))) return rc;
  // gather the rows into one buffer: one D2H copy instead of one per slot
  S_TRY(hipMemcpyAsync(d + oA, h + oA, sizeof(uint64_t) * n, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(gather_rows, dim3(n), dim3(256), 0, st, (const uint64_t*)(d + oA),
                     (double*)(d + oO), n_nodes);
  S_TRY(hipGetLastError());
  S_TRY(hipMemcpyAsync(h + oO, d + oO, bytes, hipMemcpyDeviceToHost, st));
  S_TRY(hipStreamSynchronize(st));
  memcpy(out, h + oO, bytes);
  return FDCN_OK;
}

}  // extern "C"
