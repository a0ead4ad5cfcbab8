// Room impulse responses by the image-source method (Allen & Berkley 1979, as Habets' RIR generator states it), float64,
// omnidirectional receiver.  Each batch item has its own source and receiver.  alvq_rir_f64 shares the room and the wall
// reflection coefficients across the batch; alvq_rir_rooms_f64 reads a room and six coefficients per item.  c, fs, nsample,
// order and the high-pass switch are shared.  Lengths are in samples (x / cTs, cTs = c / fs) throughout.
//
// Two kernels, no atomics, every output sample a sum in one fixed order (bitwise reproducible, independent of the batch):
//   rir_gather_kernel  output-stationary.  One workgroup = (item b, a tile of RIR_TILE output samples); lane i of every wave owns
//                      sample t0 + i.  Only images whose Tw-tap window reaches the tile can contribute, i.e. whose distance lies in
//                      a spherical shell around the receiver.  The image grid is cut into columns (m_x, q, m_y, j); for each
//                      column the two m_z intervals of each k that meet the shell are solved in closed form (widened by one), and
//                      every candidate gets the exact test.  Templated on where the room and beta come from: the launch's
//                      parameters, or the item's row of room (B,3) / beta (B,6), from which each workgroup derives the item's
//                      image ranges with the host's float64 expression (so an item's bits equal a one-room launch's).  Wave w takes the columns w*64 + lane (+ 256 per round); each
//                      sub-round every lane posts its next accepted image to its LDS slot, and the wave adds the 64 slots in
//                      slot order to its own partial.  The four partials are added in wave order at the end.
//                      Per tap there is no cos / sin: sin(pi (t-d)) = -(-1)^(t-fd) sin(pi frac) (one sinpi per image), and the
//                      window cos(2 pi (m - frac)/Tw) is the rotation of a per-launch table cos / sin(2 pi m/Tw) by frac.
//   rir_highpass_kernel  the generator's 100 Hz high-pass, a serial recurrence: one thread per response, in place, over the
//                      response staged in LDS.
#include <cfloat>
#include <climits>
#include <cmath>

#include "alvq_common.h"

namespace alvq {

constexpr int RIR_TILE = 64;       // output samples per workgroup (one per lane)
constexpr int RIR_WAVES = 4;       // waves per workgroup: each takes a quarter of the columns
constexpr int RIR_MAX_TW = 1024;   // window length limit (LDS table): fs <= 128 kHz

struct RirParams {
  double L[3];       // room, in samples
  double beta[6];
  double cTs;
  int n[3];          // image index ranges m in [-n, n]
  int ncols;         // (2n_x+1) * 2 * (2n_y+1) * 2
  int nsample, Tw, order, tiles;
};

__device__ __forceinline__ double ipow(double b, int e) {  // b^e, e >= 0, by repeated multiplication (0^0 = 1)
  double r = 1.0;
  for (int i = 0; i < e; ++i) r *= b;
  return r;
}

// The m_z range of one column and one k whose images may lie in the shell [dlo, dhi) (two intervals, by the sign of z, merged
// when they touch; widened by one so that rounding cannot lose an image -- the exact test decides).
struct ZRange {
  int lo0, hi0, lo1, hi1;
};

__device__ __forceinline__ ZRange z_ranges(double a, double twoLz, double rho2, double dlo, double dhi, int nz) {
  ZRange zr{1, 0, 1, 0};
  const double zmax2 = dhi * dhi - rho2;
  if (zmax2 < 0.0) return zr;
  const double zmax = sqrt(zmax2), zmin = sqrt(fmax(dlo * dlo - rho2, 0.0));
  // z = a + twoLz * m in [zmin, zmax] or in [-zmax, -zmin]
  int plo = (int)ceil((zmin - a) / twoLz) - 1, phi = (int)floor((zmax - a) / twoLz) + 1;
  int nlo = (int)ceil((-zmax - a) / twoLz) - 1, nhi = (int)floor((-zmin - a) / twoLz) + 1;
  plo = max(plo, -nz); phi = min(phi, nz);
  nlo = max(nlo, -nz); nhi = min(nhi, nz);
  if (nhi >= plo - 1) {                 // the intervals touch (zmin small): one range
    zr.lo0 = min(nlo, plo);
    zr.hi0 = max(nhi, phi);
  } else {
    zr.lo0 = nlo; zr.hi0 = nhi;
    zr.lo1 = plo; zr.hi1 = phi;
  }
  return zr;
}

struct Image {
  double frac, gain, sf, cw, sw;  // d - fd, refl / (4 pi d cTs), sin(pi frac), cos / sin(2 pi frac / Tw)
  int fd;
};

// Per-item status bits of alvq_rir_rooms_f64 (an item with any bit set is not summed: its response is left zero).
constexpr int RIR_BAD_BETA = 1;    // some |beta| > 1, or not a number
constexpr int RIR_BAD_ROOM = 2;    // a room side not a positive finite length, or an image range above RIR_MAX_N
constexpr double RIR_MAX_N = 4096.0;

// The image range of one axis: the generator's ceil(nsample / (2 L)), this exact float64 expression (host and device alike).
__host__ __device__ __forceinline__ double rir_image_range(int nsample, double L) { return ceil((double)nsample / (2.0 * L)); }

struct RirRooms {           // alvq_rir_rooms_f64's per-item inputs (all null for alvq_rir_f64)
  const double* room;       // (B,3) metres
  const double* beta;       // (B,6)
  int* status;              // (B,) RIR_BAD_* bits, written by the item's first tile
};

__device__ __forceinline__ double wave_uniform(double v) {   // v is the same in every lane: keep it in scalar registers
  const long long u = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readfirstlane((int)u), hi = __builtin_amdgcn_readfirstlane((int)(u >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Item b's room in samples, beta, image ranges and column count into P; returns the item's status bits.
__device__ __forceinline__ int rir_item_params(RirParams& P, const RirRooms& R, int b) {
  int st = 0;
  for (int a = 0; a < 6; ++a) {
    const double v = R.beta[6 * b + a];
    if (!(fabs(v) <= 1.0)) st |= RIR_BAD_BETA;
    P.beta[a] = v;
  }
  for (int a = 0; a < 3; ++a) {
    const double La = R.room[3 * b + a];
    P.L[a] = wave_uniform(La / P.cTs);
    const double n = rir_image_range(P.nsample, P.L[a]);
    if (!(La > 0.0 && La <= DBL_MAX && n <= RIR_MAX_N)) st |= RIR_BAD_ROOM;
    P.n[a] = (st & RIR_BAD_ROOM) ? 0 : (int)n;
  }
  P.ncols = st ? 0 : (2 * P.n[0] + 1) * 2 * (2 * P.n[1] + 1) * 2;
  return st;
}

template <bool ROOMS>
__global__ __launch_bounds__(256) void rir_gather_kernel(const double* __restrict__ src, const double* __restrict__ rcv,
                                                         double* __restrict__ h, RirParams P, RirRooms R) {
  __shared__ double tab_c[RIR_MAX_TW], tab_s[RIR_MAX_TW];     // cos / sin(2 pi m / Tw), m = n - Tw/2 + 1, n in [0, Tw)
  __shared__ double s_frac[256], s_gain[256], s_sf[256], s_cw[256], s_sw[256];
  __shared__ int s_fd[256];
  __shared__ double part[RIR_WAVES][RIR_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.x / P.tiles, t0 = (blockIdx.x % P.tiles) * RIR_TILE;
  if constexpr (ROOMS) {
    const int st = rir_item_params(P, R, b);
    if (t0 == 0 && tid == 0) R.status[b] = st;
  }
  const int Tw = P.Tw, half = Tw / 2;
  for (int n = tid; n < Tw; n += 256) {
    const double m = (double)(n - half + 1);
    tab_c[n] = cospi(2.0 * m / (double)Tw);
    tab_s[n] = sinpi(2.0 * m / (double)Tw);
  }
  __syncthreads();
  double s[3], r[3];
  for (int a = 0; a < 3; ++a) {
    s[a] = src[3 * b + a] / P.cTs;
    r[a] = rcv[3 * b + a] / P.cTs;
  }
  const int t1 = min(t0 + RIR_TILE, P.nsample);
  // an image reaches the tile iff fd in [t0 - Tw/2, t1 - 2 + Tw/2] (and fd < nsample)
  const int fd_lo = t0 - half, fd_hi = min(t1 - 2 + half, P.nsample - 1);
  const double dlo = fmax((double)fd_lo, 0.0), dhi = (double)fd_hi + 1.0;
  const int t = t0 + lane;
  double acc = 0.0;
  const int ny2 = 2 * P.n[1] + 1;
  double* slot_frac = s_frac + wv * 64;
  double* slot_gain = s_gain + wv * 64;
  double* slot_sf = s_sf + wv * 64;
  double* slot_cw = s_cw + wv * 64;
  double* slot_sw = s_sw + wv * 64;
  int* slot_fd = s_fd + wv * 64;
  for (int base = wv * 64; base < P.ncols; base += 256) {
    // this lane's column: c = ((m_x + n_x) * 2 + q) * (2 (2 n_y + 1)) + (m_y + n_y) * 2 + j
    const int c = base + lane;
    bool live = c < P.ncols;
    int mx = 0, q = 0, my = 0, jj = 0;
    if (live) {
      const int cx = c / (2 * ny2), cy = c - cx * 2 * ny2;
      mx = (cx >> 1) - P.n[0]; q = cx & 1;
      my = (cy >> 1) - P.n[1]; jj = cy & 1;
    }
    const double xc = (double)(1 - 2 * q) * s[0] - r[0] + 2.0 * (double)mx * P.L[0];
    const double yc = (double)(1 - 2 * jj) * s[1] - r[1] + 2.0 * (double)my * P.L[1];
    const double rho2 = xc * xc + yc * yc;
    const double refl_xy = ipow(P.beta[0], abs(mx - q)) * ipow(P.beta[1], abs(mx)) * ipow(P.beta[2], abs(my - jj)) *
                           ipow(P.beta[3], abs(my));
    const int ord_xy = abs(2 * mx - q) + abs(2 * my - jj);
    if (P.order >= 0 && ord_xy > P.order) live = false;
    // candidate cursor: k in {0, 1}, seg in {0, 1} (the two m_z intervals of that k)
    int k = 0, seg = 0, mz = 0, hi = -1;
    ZRange zr{1, 0, 1, 0};
    if (live) {
      zr = z_ranges((double)(1 - 2 * 0) * s[2] - r[2], 2.0 * P.L[2], rho2, dlo, dhi, P.n[2]);
      mz = zr.lo0;
      hi = zr.hi0;
    }
    while (true) {
      // advance to this lane's next accepted image
      bool has = false;
      Image im{};
      while (live) {
        if (mz > hi) {
          if (seg == 0) {
            seg = 1; mz = zr.lo1; hi = zr.hi1;
          } else if (k == 0) {
            k = 1; seg = 0;
            zr = z_ranges(-s[2] - r[2], 2.0 * P.L[2], rho2, dlo, dhi, P.n[2]);
            mz = zr.lo0; hi = zr.hi0;
          } else {
            live = false;
          }
          continue;
        }
        const int m = mz++;
        if (P.order >= 0 && ord_xy + abs(2 * m - k) > P.order) continue;
        const double zc = (double)(1 - 2 * k) * s[2] - r[2] + 2.0 * (double)m * P.L[2];
        const double d = sqrt(rho2 + zc * zc);
        const double fdd = floor(d);
        if (fdd < (double)fd_lo || fdd > (double)fd_hi) continue;
        const double refl = refl_xy * ipow(P.beta[4], abs(m - k)) * ipow(P.beta[5], abs(m));
        im.fd = (int)fdd;
        im.frac = d - fdd;
        im.gain = refl / (4.0 * M_PI * d * P.cTs);
        im.sf = sinpi(im.frac);
        im.cw = cospi(2.0 * im.frac / (double)Tw);
        im.sw = sinpi(2.0 * im.frac / (double)Tw);
        has = true;
        break;
      }
      if (__ballot(has) == 0) break;   // wave-uniform: no lane of this wave has an image left in this round
      slot_fd[lane] = has ? im.fd : INT_MIN / 2;
      slot_frac[lane] = im.frac;
      slot_gain[lane] = im.gain;
      slot_sf[lane] = im.sf;
      slot_cw[lane] = im.cw;
      slot_sw[lane] = im.sw;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      for (int e = 0; e < 64; ++e) {
        const int fd = slot_fd[e];
        const int n = t - fd + half - 1;   // tap index of sample t in this image's window
        if (n < 0 || n >= Tw) continue;     // also skips empty slots (fd = INT_MIN / 2)
        const double frac = slot_frac[e];
        const int m = t - fd;
        const double u = (double)m - frac;
        const double w = 0.5 * (1.0 + (tab_c[n] * slot_cw[e] + tab_s[n] * slot_sw[e]));
        double sinc = 1.0;
        if (u != 0.0) {
          const double sf = slot_sf[e];
          sinc = ((m & 1) ? sf : -sf) / (M_PI * u);
        }
        acc += slot_gain[e] * (w * sinc);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
  }
  part[wv][lane] = acc;
  __syncthreads();
  if (wv == 0 && t < P.nsample) h[(long)b * P.nsample + t] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// y0 = B1 y1 + B2 y2 + x_t;  h_t = y0 + A1 y1 + R1 y2   (lfilter([1, A1, R1], [1, -B1, -B2])).  One workgroup per response: the
// workgroup stages RIR_HP_CHUNK samples in LDS, thread 0 runs the recurrence over them, the workgroup writes them back, so the
// serial chain never waits on a global load.
constexpr int RIR_HP_CHUNK = 4096;
__global__ __launch_bounds__(256) void rir_highpass_kernel(double* __restrict__ h, int nsample, double fs) {
  __shared__ double buf[RIR_HP_CHUNK];
  const int tid = threadIdx.x;
  const double W = 2.0 * M_PI * 100.0 / fs, R1 = exp(-W), B1 = 2.0 * R1 * cos(W), B2 = -R1 * R1, A1 = -(1.0 + R1);
  double* x = h + (long)blockIdx.x * nsample;
  double y1 = 0.0, y2 = 0.0;
  for (int c0 = 0; c0 < nsample; c0 += RIR_HP_CHUNK) {
    const int n = min(RIR_HP_CHUNK, nsample - c0);
    for (int i = tid; i < n; i += 256) buf[i] = x[c0 + i];
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < n; ++i) {
        const double y0 = B1 * y1 + B2 * y2 + buf[i];
        buf[i] = y0 + A1 * y1 + R1 * y2;
        y2 = y1;
        y1 = y0;
      }
    __syncthreads();
    for (int i = tid; i < n; i += 256) x[c0 + i] = buf[i];
    __syncthreads();
  }
}

}  // namespace alvq

using namespace alvq;

// The arguments both entry points share, checked before any launch, into P (everything but L, beta, n and ncols).
static int rir_shared_params(const char* who, const double* src, const double* rcv, double* h, int B, int nsample, double c,
                             double fs, int order, int hp_filter, RirParams& P) {
  ALVQ_REQUIRE(src && rcv && h, ALVQ_EINVAL, "%s: null pointer", who);
  ALVQ_REQUIRE(B > 0 && nsample > 0 && nsample <= (1 << 24), ALVQ_EINVAL, "%s: B=%d nsample=%d (need B > 0, 0 < nsample <= 2^24)",
               who, B, nsample);
  ALVQ_REQUIRE(std::isfinite(c) && c > 0.0 && std::isfinite(fs) && fs > 0.0, ALVQ_EINVAL, "%s: c=%g fs=%g must be > 0", who, c, fs);
  ALVQ_REQUIRE(order >= -1, ALVQ_EINVAL, "%s: order=%d (need >= -1)", who, order);
  ALVQ_REQUIRE(hp_filter == 0 || hp_filter == 1, ALVQ_EINVAL, "%s: hp_filter=%d (need 0 or 1)", who, hp_filter);
  P.cTs = c / fs;
  P.Tw = 2 * (int)floor(0.004 * fs + 0.5);
  ALVQ_REQUIRE(P.Tw >= 2 && P.Tw <= RIR_MAX_TW, ALVQ_EINVAL, "%s: fs=%g gives a %d-tap window (need 2..%d)", who, fs, P.Tw,
               RIR_MAX_TW);
  P.nsample = nsample;
  P.order = order;
  P.tiles = (nsample + RIR_TILE - 1) / RIR_TILE;
  ALVQ_REQUIRE((long)B * P.tiles < (1L << 31), ALVQ_EINVAL, "%s: B=%d x %d tiles too many workgroups", who, B, P.tiles);
  return ALVQ_OK;
}

extern "C" int alvq_rir_f64(const double* src, const double* rcv, double* h, int B, int nsample, double Lx, double Ly, double Lz,
                            const double* beta6_host, double c, double fs, int order, int hp_filter, void* stream) {
  const char* who = "alvq_rir_f64";
  ALVQ_REQUIRE(beta6_host, ALVQ_EINVAL, "%s: null pointer", who);
  RirParams P;
  const int rc = rir_shared_params(who, src, rcv, h, B, nsample, c, fs, order, hp_filter, P);
  if (rc != ALVQ_OK) return rc;
  ALVQ_REQUIRE(std::isfinite(Lx) && std::isfinite(Ly) && std::isfinite(Lz) && Lx > 0.0 && Ly > 0.0 && Lz > 0.0, ALVQ_EINVAL,
               "%s: room %g x %g x %g must be > 0", who, Lx, Ly, Lz);
  for (int a = 0; a < 6; ++a) {
    ALVQ_REQUIRE(std::isfinite(beta6_host[a]) && fabs(beta6_host[a]) <= 1.0, ALVQ_EINVAL, "%s: beta[%d]=%g (need |beta| <= 1)",
                 who, a, beta6_host[a]);
    P.beta[a] = beta6_host[a];
  }
  const double Ls[3] = {Lx / P.cTs, Ly / P.cTs, Lz / P.cTs};
  for (int a = 0; a < 3; ++a) {
    P.L[a] = Ls[a];
    const double n = rir_image_range(nsample, Ls[a]);
    ALVQ_REQUIRE(n <= RIR_MAX_N, ALVQ_EINVAL, "%s: nsample=%d spans %g rooms along axis %d (limit 4096)", who, nsample, n, a);
    P.n[a] = (int)n;
  }
  P.ncols = (2 * P.n[0] + 1) * 2 * (2 * P.n[1] + 1) * 2;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rir_gather_kernel<false>, dim3(B * P.tiles), dim3(256), 0, s, src, rcv, h, P, RirRooms{nullptr, nullptr, nullptr});
  if (hp_filter) hipLaunchKernelGGL(rir_highpass_kernel, dim3(B), dim3(256), 0, s, h, nsample, fs);
  return check_launch(who);
}

extern "C" int alvq_rir_rooms_f64(const double* src, const double* rcv, const double* room, const double* beta, double* h,
                                  int* status, int B, int nsample, double c, double fs, int order, int hp_filter, void* stream) {
  const char* who = "alvq_rir_rooms_f64";
  ALVQ_REQUIRE(room && beta && status, ALVQ_EINVAL, "%s: null pointer", who);
  RirParams P;
  const int rc = rir_shared_params(who, src, rcv, h, B, nsample, c, fs, order, hp_filter, P);
  if (rc != ALVQ_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rir_gather_kernel<true>, dim3(B * P.tiles), dim3(256), 0, s, src, rcv, h, P, RirRooms{room, beta, status});
  if (hp_filter) hipLaunchKernelGGL(rir_highpass_kernel, dim3(B), dim3(256), 0, s, h, nsample, fs);
  return check_launch(who);
}
