// Eddy-viscosity kernels: cmpt_sgs (reference src/sgs.f90:21-386) for 'smag' (van Driest damped) and
// 'dsmag' (dynamic, plane-averaged: the reference hard-wires _CHANNEL, sgs.f90:8,362-364; averaged over the volume, over x lines or not at all -- _DIT,
// _DUCT, _CAVITY, sgs.f90:359-370 -- under the flags of cales_case.sgstype, SgsAve), with
// strain_rate (sgs.f90:1019-1110), extrapolate (682-767), filter3d (616-680), interpolate (850-870),
// ave1d_channel (433-482) and cmpt_alph2 (769-822).
#include "common.hpp"
#include <type_traits>

#define BX 64
#define BY 4

// ------------------------------------------------------------------------------------------ extrapolate
struct ExJob { real *p; int idir, ibound; real factor; real *save; int restore; };   // save: plane buffer for the overwritten ghosts
struct ExJobs { int njobs; ExJob job[18]; };
__global__ __launch_bounds__(256) void k_extrapolate(Geom g, ExJobs J) {
  const ExJob jb = J.job[blockIdx.z];
  const int idir = jb.idir;
  const int na = idir == 1 ? g.n2 : g.n1, nb = idir == 3 ? g.n2 : g.n3, n = idir == 1 ? g.n1 : idir == 2 ? g.n2 : g.n3;
  const int a = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y * 4 + threadIdx.y;
  if (a > na + 1 || b > nb + 1) return;
  const long st = idir == 1 ? 1 : idir == 2 ? (long)g.s1 : g.s12;
  real *p = jb.p + (idir == 1 ? g.ix(0, a, b) : idir == 2 ? g.ix(a, 0, b) : g.ix(a, b, 0));
#define P(m) p[(long)(m)*st]
  const real f = jb.factor;
  const int gh = jb.ibound == 0 ? 0 : n + 1;
  if (jb.save) {                      // in-place use on a live field: keep / give back the ghost value
    const size_t q = (size_t)a + (size_t)(na + 2) * b;
    if (jb.restore) { P(gh) = jb.save[q]; return; }
    jb.save[q] = P(gh);
  }
  if (idir < 3) { if (jb.ibound == 0) P(0) = 2. * P(1) - P(2); else P(n + 1) = 2. * P(n) - P(n - 1); }
  else { if (jb.ibound == 0) P(0) = (1. + f) * P(1) - f * P(2); else P(n + 1) = (1. + f) * P(n) - f * P(n - 1); }
#undef P
}
// mode 0: `lwm` form (wall-model faces, z factors from the grid), 1: `cbc` form (all no-slip walls, factor 1)
// save != nullptr: the fields are live (u,v,w themselves): the ghosts they lose are kept in `save` (restore = 0) and given back
// afterwards (restore = 1, directions in reverse order so that edge cells see the same sequence backwards)
static int extrapolate(cales_ctx *c, int nf, real **p, const int *iface, int mode, real *save = nullptr, int restore = 0) {
  const int *n = c->n;
  // save slots: [direction][field][side], each the size of that direction's ghost plane
  const size_t psz[3] = {(size_t)(n[1] + 2) * (n[2] + 2), (size_t)(n[0] + 2) * (n[2] + 2), (size_t)(n[0] + 2) * (n[1] + 2)};
  const size_t poff[3] = {0, 6 * psz[0], 6 * (psz[0] + psz[1])};
  for (int step = 1; step <= 3; ++step) {      // one launch per direction, order x,y,z as the reference
    const int idir = restore ? 4 - step : step;
    ExJobs J; J.njobs = 0;
    for (int q = 0; q < nf; ++q) for (int ib = 0; ib <= 1; ++ib) {
      bool done;
      real factor = 1.;
      if (mode == 1) done = ISB(c, ib, idir) && CBV(c, ib, idir, idir) == 'D' && iface[q] != idir;
      else {
        done = ISB(c, ib, idir) && LWM(c, ib, idir) != 0 && iface[q] != idir;
        factor = ib == 0 ? (1. / c->dzci[0]) * c->dzci[1] : (1. / c->dzci[n[2]]) * c->dzci[n[2] - 1];
      }
      if (!done) continue;
      ExJob &j = J.job[J.njobs++]; j.p = p[q]; j.idir = idir; j.ibound = ib; j.factor = factor; j.save = nullptr; j.restore = restore;
      if (save) j.save = save + poff[idir - 1] + (size_t)(q * 2 + ib) * psz[idir - 1];
    }
    if (!J.njobs) continue;
    const int na = idir == 1 ? n[1] : n[0], nb = idir == 3 ? n[1] : n[2];
    LAUNCH(c, k_extrapolate, dim3((na + 2 + 63) / 64, (nb + 2 + 3) / 4, J.njobs), dim3(64, 4), 0, c->stream, c->g, J);
  }
  LAUNCHCHK(c);
  return 0;
}

// ------------------------------------------------------------------------------------------ strain_rate
template <int WITH_SIJ>
__global__ __launch_bounds__(BX *BY) void k_strain(Geom g, real dxi, real dyi, const real *__restrict__ dzci,
                                                    const real *__restrict__ dzfi, const real *__restrict__ u,
                                                    const real *__restrict__ v, const real *__restrict__ w, real *__restrict__ s0,
                                                    real *__restrict__ s11o, real *__restrict__ s22o, real *__restrict__ s33o,
                                                    real *__restrict__ s12o, real *__restrict__ s13o, real *__restrict__ s23o) {
  int bx_, by_, bz_; stencil_block(bx_, by_, bz_);
  const int i = bx_ * BX + threadIdx.x + 1, j = by_ * BY + threadIdx.y + 1, k = bz_ + 1;
  if (i > g.n1 || j > g.n2) return;
  const size_t c = g.ix(i, j, k);
  const long sj = g.s1, sk = g.s12;
#define LD(a, di, dj, dk) a[c + (di) + (dj)*sj + (dk)*sk]
  const real u_mcm = LD(u, -1, 0, -1), u_ccm = LD(u, 0, 0, -1), u_mmc = LD(u, -1, -1, 0), u_cmc = LD(u, 0, -1, 0), u_mcc = LD(u, -1, 0, 0),
               u_ccc = LD(u, 0, 0, 0), u_mpc = LD(u, -1, 1, 0), u_cpc = LD(u, 0, 1, 0), u_mcp = LD(u, -1, 0, 1), u_ccp = LD(u, 0, 0, 1);
  const real v_cmm = LD(v, 0, -1, -1), v_ccm = LD(v, 0, 0, -1), v_mmc = LD(v, -1, -1, 0), v_cmc = LD(v, 0, -1, 0), v_pmc = LD(v, 1, -1, 0),
               v_mcc = LD(v, -1, 0, 0), v_ccc = LD(v, 0, 0, 0), v_pcc = LD(v, 1, 0, 0), v_cmp = LD(v, 0, -1, 1), v_ccp = LD(v, 0, 0, 1);
  const real w_cmm = LD(w, 0, -1, -1), w_mcm = LD(w, -1, 0, -1), w_ccm = LD(w, 0, 0, -1), w_pcm = LD(w, 1, 0, -1), w_cpm = LD(w, 0, 1, -1),
               w_cmc = LD(w, 0, -1, 0), w_mcc = LD(w, -1, 0, 0), w_ccc = LD(w, 0, 0, 0), w_pcc = LD(w, 1, 0, 0), w_cpc = LD(w, 0, 1, 0);
#undef LD
  const real zc = dzci[k], zm = dzci[k - 1];
  const real s11 = (u_ccc - u_mcc) * dxi, s22 = (v_ccc - v_cmc) * dyi, s33 = (w_ccc - w_ccm) * dzfi[k];
  const real s12 = .125 * ((u_cpc - u_ccc) * dyi + (v_pcc - v_ccc) * dxi + (u_ccc - u_cmc) * dyi + (v_pmc - v_cmc) * dxi +
                             (u_mpc - u_mcc) * dyi + (v_ccc - v_mcc) * dxi + (u_mcc - u_mmc) * dyi + (v_cmc - v_mmc) * dxi);
  const real s13 = .125 * ((u_ccp - u_ccc) * zc + (w_pcc - w_ccc) * dxi + (u_ccc - u_ccm) * zm + (w_pcm - w_ccm) * dxi +
                             (u_mcp - u_mcc) * zc + (w_ccc - w_mcc) * dxi + (u_mcc - u_mcm) * zm + (w_ccm - w_mcm) * dxi);
  const real s23 = .125 * ((v_ccp - v_ccc) * zc + (w_cpc - w_ccc) * dyi + (v_ccc - v_ccm) * zm + (w_cpm - w_ccm) * dyi +
                             (v_cmp - v_cmc) * zc + (w_ccc - w_cmc) * dyi + (v_cmc - v_cmm) * zm + (w_ccm - w_cmm) * dyi);
  const real s0v = sqrt(2. * (s11 * s11 + s22 * s22 + s33 * s33 + 2. * (s12 * s12 + s13 * s13 + s23 * s23)));
  s0[c] = s0v;
  if (WITH_SIJ) { s11o[c] = s11; s22o[c] = s22; s33o[c] = s33; s12o[c] = s12; s13o[c] = s13; s23o[c] = s23; }
}
static int strain_rate(cales_ctx *c, const real *u, const real *v, const real *w, real *s0, real **sij) {
  ProfScope ps(c, "strain_rate");
  dim3 b(BX, BY, 1), gr = grid3(c->n[0], c->n[1], c->n[2], b);
  if (sij) LAUNCH(c, k_strain<1>, gr, b, 0, c->stream, c->g, c->dli[0], c->dli[1], c->d_dzci, c->d_dzfi, u, v, w, s0, sij[0], sij[1], sij[2], sij[3], sij[4], sij[5]);
  else LAUNCH(c, k_strain<0>, gr, b, 0, c->stream, c->g, c->dli[0], c->dli[1], c->d_dzci, c->d_dzfi, u, v, w, s0, (real *)nullptr,
                          (real *)nullptr, (real *)nullptr, (real *)nullptr, (real *)nullptr, (real *)nullptr);
  LAUNCHCHK(c);
  return 0;
}

// ------------------------------------------------------------------------------------------ static Smagorinsky (sgs.f90:98-152)
struct SmagArgs { real w0, w1, w2, w3, w4, w5, dl1, dl2, l3, dxi, dyi, visc, sumw; };
__global__ __launch_bounds__(BX *BY) void k_smag(Geom g, SmagArgs A, const real *__restrict__ zc, const real *__restrict__ dzci,
                                                  const real *__restrict__ dzf, const real *__restrict__ u, const real *__restrict__ v,
                                                  const real *__restrict__ w, const real *__restrict__ s0, real *__restrict__ visct,
                                                  const real *__restrict__ twy) {      // twy != null (several slabs): sqrt(tau_w) planes of the two y walls, see wall_shear_y_planes
  int bx_, by_, bz_; stencil_block(bx_, by_, bz_);
  const int i = bx_ * BX + threadIdx.x + 1, j = by_ * BY + threadIdx.y + 1, k = bz_ + 1;
  if (i > g.n1 || j > g.n2) return;
  real fd;
  if (A.sumw == 0.) fd = 1.;
  else {
    const int jg = j + g.jlo;                    // global row: distances to the y walls use global indices
    real dw[6];
    dw[0] = A.dl1 * (i - 0.5); dw[1] = A.dl1 * (g.n1 - i + 0.5);
    dw[2] = A.dl2 * (jg - 0.5); dw[3] = A.dl2 * (g.ng2 - jg + 0.5);
    dw[4] = zc[k]; dw[5] = A.l3 - zc[k];
    const real isw[6] = {A.w0, A.w1, A.w2, A.w3, A.w4, A.w5};
    int loc = 0;
#pragma unroll
    for (int q = 0; q < 6; ++q) dw[q] = dw[q] * isw[q] + CALES_BIG * (1. - isw[q]);
#pragma unroll
    for (int q = 1; q < 6; ++q) if (dw[q] < dw[loc]) loc = q;
    const real dw_min = dw[loc];
    real t1 = 0., t2 = 0., sc = 0.;
    const int n1 = g.n1, n2 = g.n2, n3 = g.n3, im1 = i - 1;
    if (twy && (loc == 2 || loc == 3)) {      // the y walls belong to the first and the last slab: their shear arrives as planes (same arithmetic, k_wall_shear_y)
      const real dw_plus = dw_min * twy[(size_t)(loc == 2 ? k : n3 + 2 + k) * g.s1 + i] * (1. / A.visc);
      fd = 1. - exp(-dw_plus / 25.);
    } else {
    switch (loc) {
    case 0: t1 = v[g.ix(1, j, k)] - v[g.ix(0, j, k)] + v[g.ix(1, j - 1, k)] - v[g.ix(0, j - 1, k)];
            t2 = w[g.ix(1, j, k)] - w[g.ix(0, j, k)] + w[g.ix(1, j, k - 1)] - w[g.ix(0, j, k - 1)]; sc = A.dxi; break;
    case 1: t1 = v[g.ix(n1, j, k)] - v[g.ix(n1 + 1, j, k)] + v[g.ix(n1, j - 1, k)] - v[g.ix(n1 + 1, j - 1, k)];
            t2 = w[g.ix(n1, j, k)] - w[g.ix(n1 + 1, j, k)] + w[g.ix(n1, j, k - 1)] - w[g.ix(n1 + 1, j, k - 1)]; sc = A.dxi; break;
    case 2: t1 = u[g.ix(i, 1, k)] - u[g.ix(i, 0, k)] + u[g.ix(i - 1, 1, k)] - u[g.ix(i - 1, 0, k)];
            t2 = w[g.ix(i, 1, k)] - w[g.ix(i, 0, k)] + w[g.ix(i, 1, k - 1)] - w[g.ix(i, 0, k - 1)]; sc = A.dyi; break;
    case 3: t1 = u[g.ix(i, n2, k)] - u[g.ix(i, n2 + 1, k)] + u[g.ix(i - 1, n2, k)] - u[g.ix(i - 1, n2 + 1, k)];
            t2 = w[g.ix(i, n2, k)] - w[g.ix(i, n2 + 1, k)] + w[g.ix(i, n2, k - 1)] - w[g.ix(i, n2 + 1, k - 1)]; sc = A.dyi; break;
    case 4: t1 = u[g.ix(i, j, 1)] - u[g.ix(i, j, 0)] + u[g.ix(im1, j, 1)] - u[g.ix(im1, j, 0)];
            t2 = v[g.ix(i, j, 1)] - v[g.ix(i, j, 0)] + v[g.ix(i, j - 1, 1)] - v[g.ix(i, j - 1, 0)]; sc = dzci[0]; break;
    default: t1 = u[g.ix(i, j, n3)] - u[g.ix(i, j, n3 + 1)] + u[g.ix(im1, j, n3)] - u[g.ix(im1, j, n3 + 1)];
             t2 = v[g.ix(i, j, n3)] - v[g.ix(i, j, n3 + 1)] + v[g.ix(i, j - 1, n3)] - v[g.ix(i, j - 1, n3 + 1)]; sc = dzci[n3]; break;
    }
    real tauw_s = sqrt(t1 * t1 + t2 * t2) * sc;
    tauw_s = 0.5 * A.visc * tauw_s;
    const real dw_plus = dw_min * sqrt(tauw_s) * (1. / A.visc);
    fd = 1. - exp(-dw_plus / 25.);
    }
  }
  const real t = 0.11 * dzf[k] * fd;        // dzf[] here is the table (dx dy dzf(k))^(1/3) of k_smag_del (sgs.f90:145); c_smag, src/param.f90:33
  const size_t c = g.ix(i, j, k);
  visct[c] = (t * t) * s0[c];
}

// ------------------------------------------------------------------------------------------ small dsmag kernels
__global__ __launch_bounds__(256) void k_copy3(size_t n, const real *__restrict__ a, const real *__restrict__ b, const real *__restrict__ c_,
                                               real *__restrict__ x, real *__restrict__ y, real *__restrict__ z) {
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) { x[q] = a[q]; y[q] = b[q]; z[q] = c_[q]; }
}
__global__ __launch_bounds__(256) void k_copy1(size_t n, const real *__restrict__ a, real *__restrict__ x) {
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) x[q] = a[q];
}
struct P6 { real *p[6]; };
struct CP6 { const real *p[6]; };
__global__ __launch_bounds__(256) void k_s0sij(size_t n, const real *__restrict__ s0, CP6 sij, P6 wk) {   // sgs.f90:198-210 (all cells)
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) {
    const real s = s0[q];
#pragma unroll
    for (int m = 0; m < 6; ++m) wk.p[m][q] = s * sij.p[m][q];
  }
}
__global__ __launch_bounds__(256) void k_uiuj(size_t n, const real *__restrict__ uc, const real *__restrict__ vc, const real *__restrict__ wc, P6 wk) {
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) {   // sgs.f90:283-295
    const real a = uc[q], b = vc[q], c_ = wc[q];
    wk.p[0][q] = a * a; wk.p[1][q] = b * b; wk.p[2][q] = c_ * c_; wk.p[3][q] = a * b; wk.p[4][q] = a * c_; wk.p[5][q] = b * c_;
  }
}
// filter3d (sgs.f90:632-679): 27-point top-hat, weights 8/4/2/1 over 64
__global__ __launch_bounds__(BX *BY) void k_filter3d(Geom g, const real *__restrict__ p, real *__restrict__ pf) {
  int bx_, by_, bz_; stencil_block(bx_, by_, bz_);
  const int i = bx_ * BX + threadIdx.x + 1, j = by_ * BY + threadIdx.y + 1, k = bz_ + 1;
  if (i > g.n1 || j > g.n2) return;
  const size_t c = g.ix(i, j, k);
  const long sj = g.s1, sk = g.s12;
#define Q(di, dj, dk) p[c + (di) + (dj)*sj + (dk)*sk]
  pf[c] = (8. * (Q(0, 0, 0)) + 4. * (Q(-1, 0, 0) + Q(0, -1, 0) + Q(0, 0, -1) + Q(1, 0, 0) + Q(0, 1, 0) + Q(0, 0, 1)) +
           2. * (Q(0, -1, -1) + Q(-1, 0, -1) + Q(-1, -1, 0) + Q(0, 1, -1) + Q(1, 0, -1) + Q(1, -1, 0) + Q(0, -1, 1) + Q(-1, 0, 1) +
                 Q(-1, 1, 0) + Q(0, 1, 1) + Q(1, 0, 1) + Q(1, 1, 0)) +
           1. * (Q(-1, -1, -1) + Q(1, -1, -1) + Q(-1, 1, -1) + Q(1, 1, -1) + Q(-1, -1, 1) + Q(1, -1, 1) + Q(-1, 1, 1) + Q(1, 1, 1))) / 64.;
#undef Q
}
// filter2d (sgs.f90:839-847, the -D_FILTER_2D build): 9-point top-hat in the x-y plane, weights 4/2/1 over 16, the reference's expression order
__global__ __launch_bounds__(BX *BY) void k_filter2d(Geom g, const real *__restrict__ p, real *__restrict__ pf) {
  int bx_, by_, bz_; stencil_block(bx_, by_, bz_);
  const int i = bx_ * BX + threadIdx.x + 1, j = by_ * BY + threadIdx.y + 1, k = bz_ + 1;
  if (i > g.n1 || j > g.n2) return;
  const size_t c = g.ix(i, j, k);
  const long sj = g.s1;
#define Q(di, dj) p[c + (di) + (dj)*sj]
  pf[c] = (4. * (Q(0, 0)) + 2. * (Q(-1, 0) + Q(0, -1) + Q(1, 0) + Q(0, 1)) + 1. * (Q(-1, -1) + Q(1, -1) + Q(-1, 1) + Q(1, 1))) / 16.;
#undef Q
}
// k_mij with one filter ratio for all cells (alph2 = 2.52 of the -D_FILTER_2D build, sgs.f90:817-821): no field to read
__global__ __launch_bounds__(BX *BY) void k_mij_a2(Geom g, P6 mij, real a, const real *__restrict__ s0, CP6 sij) {
  const int i = blockIdx.x * BX + threadIdx.x + 1, j = blockIdx.y * BY + threadIdx.y + 1, k = blockIdx.z + 1;   // sgs.f90:262-272
  if (i > g.n1 || j > g.n2) return;
  const size_t c = g.ix(i, j, k);
  const real s = s0[c];
#pragma unroll
  for (int m = 0; m < 6; ++m) mij.p[m][c] = 2. * (mij.p[m][c] - a * s * sij.p[m][c]);
}
__global__ __launch_bounds__(BX *BY) void k_mij(Geom g, P6 mij, const real *__restrict__ alph2, const real *__restrict__ s0, CP6 sij) {
  const int i = blockIdx.x * BX + threadIdx.x + 1, j = blockIdx.y * BY + threadIdx.y + 1, k = blockIdx.z + 1;   // sgs.f90:262-272
  if (i > g.n1 || j > g.n2) return;
  const size_t c = g.ix(i, j, k);
  const real a = alph2[c], s = s0[c];
#pragma unroll
  for (int m = 0; m < 6; ++m) mij.p[m][c] = 2. * (mij.p[m][c] - a * s * sij.p[m][c]);
}
__global__ __launch_bounds__(BX *BY) void k_interp(Geom g, const real *__restrict__ u, const real *__restrict__ v, const real *__restrict__ w,
                                                    real *__restrict__ uc, real *__restrict__ vc, real *__restrict__ wc) {
  const int i = blockIdx.x * BX + threadIdx.x + 1, j = blockIdx.y * BY + threadIdx.y + 1, k = blockIdx.z + 1;   // sgs.f90:860-869
  if (i > g.n1 || j > g.n2) return;
  const size_t c = g.ix(i, j, k);
  uc[c] = 0.5 * (u[c] + u[c - 1]); vc[c] = 0.5 * (v[c] + v[c - g.s1]); wc[c] = 0.5 * (w[c] + w[c - g.s12]);
}
__global__ __launch_bounds__(BX *BY) void k_contract(Geom g, CP6 mij, CP6 lij, const real *__restrict__ uf, const real *__restrict__ vf,
                                                      const real *__restrict__ wf, real *__restrict__ lm, real *__restrict__ mm) {
  const int i = blockIdx.x * BX + threadIdx.x + 1, j = blockIdx.y * BY + threadIdx.y + 1, k = blockIdx.z + 1;   // sgs.f90:328-358
  if (i > g.n1 || j > g.n2) return;
  const size_t c = g.ix(i, j, k);
  real m_[6], l_[6];
#pragma unroll
  for (int m = 0; m < 6; ++m) { m_[m] = mij.p[m][c]; l_[m] = lij.p[m][c]; }
  const real a = uf[c], b = vf[c], d = wf[c];
  l_[0] -= a * a; l_[1] -= b * b; l_[2] -= d * d; l_[3] -= a * b; l_[4] -= a * d; l_[5] -= b * d;
  lm[c] = m_[0] * l_[0] + m_[1] * l_[1] + m_[2] * l_[2] + (m_[3] * l_[3] + m_[4] * l_[4] + m_[5] * l_[5]) * 2.;
  mm[c] = m_[0] * m_[0] + m_[1] * m_[1] + m_[2] * m_[2] + (m_[3] * m_[3] + m_[4] * m_[4] + m_[5] * m_[5]) * 2.;
}
// The reference's _CAVITY (SgsAve::local, sgs.f90:328-358,368-377): nothing is averaged -- the two contractions of k_contract, its expressions in their
// order, and visct = max(visct * LM / MM, 0) of the very cell in one pass; the two fields between them are neither stored nor read back, nothing is
// summed and nothing travels between slabs. 16 words per cell in (visct holds |S|, sgs.f90:184), one out. A cell with MM = 0 (and so LM = 0) gives 0:
// fmax(NaN, 0) = 0, as in k_dsmag_final; the reference's max(NaN, 0) depends on its compiler, and no cell of the goldens is such a cell.
__global__ __launch_bounds__(BX *BY) void k_contract_local(Geom g, CP6 mij, CP6 lij, const real *__restrict__ uf, const real *__restrict__ vf,
                                                            const real *__restrict__ wf, real *visct) {
  const int i = blockIdx.x * BX + threadIdx.x + 1, j = blockIdx.y * BY + threadIdx.y + 1, k = blockIdx.z + 1;
  if (i > g.n1 || j > g.n2) return;
  const size_t c = g.ix(i, j, k);
  real m_[6], l_[6];
#pragma unroll
  for (int m = 0; m < 6; ++m) { m_[m] = mij.p[m][c]; l_[m] = lij.p[m][c]; }
  const real a = uf[c], b = vf[c], d = wf[c];
  l_[0] -= a * a; l_[1] -= b * b; l_[2] -= d * d; l_[3] -= a * b; l_[4] -= a * d; l_[5] -= b * d;
  const real lm = m_[0] * l_[0] + m_[1] * l_[1] + m_[2] * l_[2] + (m_[3] * l_[3] + m_[4] * l_[4] + m_[5] * l_[5]) * 2.;
  const real mm = m_[0] * m_[0] + m_[1] * m_[1] + m_[2] * m_[2] + (m_[3] * m_[3] + m_[4] * m_[4] + m_[5] * m_[5]) * 2.;
  real vt = visct[c] * lm / mm;
  visct[c] = fmax(vt, 0.);
}
// ave1d_channel (sgs.f90:462-480): plane sums of two fields -> p1d(2, n3); one block per (k, field)
__global__ __launch_bounds__(256) void k_plane_sum(Geom g, const real *__restrict__ a, const real *__restrict__ b, real *__restrict__ p1d) {
  __shared__ real sh[4];
  const int k = blockIdx.x + 1; const real *p = blockIdx.y ? b : a;
  real acc = 0.;
  const long np = (long)g.n1 * g.n2;
  for (long q = threadIdx.x; q < np; q += 256) acc += p[g.ix((int)(q % g.n1) + 1, (int)(q / g.n1) + 1, k)];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) p1d[blockIdx.y * g.n3 + blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}
// ave2d_duct(...,1,...) of the two contractions (sgs.f90:328-358,585-612; SgsAve::xlines) without the two fields between them: one wave per x line (j, k),
// four lines per block. The lanes walk the row in segments of 64 cells from i = 1 -- rows start on a 128-B line there, every load is whole lines -- with
// the expressions of k_contract in their order, each lane adding its cells in segment order; one DPP sum over the wave, and lane 63 stores the two sums
// of the line: lines[(k-1) n2 + j-1] and lines[n2 n3 + ...]. 15 words per cell are read and nothing else is written. Loads are unconditional: a lane
// past n1 reads cell n1 again and adds zero. No LDS, no barrier (a wave without a line leaves at once).
__global__ __launch_bounds__(256) void k_contract_lines(Geom g, CP6 mij, CP6 lij, const real *__restrict__ uf, const real *__restrict__ vf,
                                                        const real *__restrict__ wf, real *__restrict__ lines) {
  const int nl = g.n2 * g.n3, line = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (line >= nl) return;
  const size_t row = g.ix(0, line % g.n2 + 1, line / g.n2 + 1);
  real slm = 0., smm = 0.;
  for (int i0 = 1; i0 <= g.n1; i0 += 64) {
    const bool in = i0 + lane <= g.n1;
    const size_t c = row + (in ? i0 + lane : g.n1);
    real m_[6], l_[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) { m_[m] = mij.p[m][c]; l_[m] = lij.p[m][c]; }
    const real a = uf[c], b = vf[c], d = wf[c];
    l_[0] -= a * a; l_[1] -= b * b; l_[2] -= d * d; l_[3] -= a * b; l_[4] -= a * d; l_[5] -= b * d;
    const real lm = m_[0] * l_[0] + m_[1] * l_[1] + m_[2] * l_[2] + (m_[3] * l_[3] + m_[4] * l_[4] + m_[5] * l_[5]) * 2.;
    const real mm = m_[0] * m_[0] + m_[1] * m_[1] + m_[2] * m_[2] + (m_[3] * m_[3] + m_[4] * m_[4] + m_[5] * m_[5]) * 2.;
    slm += in ? lm : (real)0.; smm += in ? mm : (real)0.;
  }
  slm = wave_sum_lane63(slm); smm = wave_sum_lane63(smm);
  if (lane == 63) { lines[line] = slm; lines[nl + line] = smm; }
}
// visct = max(visct*<LM>(j,k)/<MM>(j,k),0) (sgs.f90:372-380 behind ave2d_duct: gar = dl(1)/l(1), sgs.f90:586,609); the line sums replace the broadcast arrays
__global__ __launch_bounds__(BX *BY) void k_dsmag_final_lines(Geom g, real gar, const real *__restrict__ lines, const real *s0, real *visct) {
  const int i = blockIdx.x * BX + threadIdx.x + 1, j = blockIdx.y * BY + threadIdx.y + 1, k = blockIdx.z + 1;
  if (i > g.n1 || j > g.n2) return;
  const size_t c = g.ix(i, j, k);
  const int q = (k - 1) * g.n2 + j - 1;
  const real lm = lines[q] * gar, mm = lines[g.n2 * g.n3 + q] * gar;
  real vt = s0[c] * lm / mm;
  visct[c] = fmax(vt, 0.);
}
// ave0d_dit (sgs.f90:388-431; SgsAve::volume) from the plane sums: T = sum over k of p1d(k) dzf(k) of both quantities, written into every plane's slot, so
// that k_dsmag_coef / k_dsmag_final run as they are (only the ratio enters: gar and 1/l(3) cancel). One block, fixed order; on several slabs every
// rank folds the same all-reduced vector. All reads of p1d precede the barrier, all writes follow it.
__global__ __launch_bounds__(256) void k_volume_fold(int n3, const real *__restrict__ dzf, real *p1d) {
  __shared__ real sh[2][4];
  real a = 0., b = 0.;
  for (int k = threadIdx.x; k < n3; k += 256) { const real d = dzf[k + 1]; a += p1d[k] * d; b += p1d[n3 + k] * d; }
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); b += __shfl_down(b, o, 64); }
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = a; sh[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  const real ta = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3], tb = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
  for (int k = threadIdx.x; k < n3; k += 256) { p1d[k] = ta; p1d[n3 + k] = tb; }
}
// visct = max(visct*<LM>/<MM>,0) (sgs.f90:372-380); the plane averages replace the broadcast arrays
__global__ __launch_bounds__(BX *BY) void k_dsmag_final(Geom g, real gar, const real *__restrict__ p1d, const real *s0, real *visct) {
  const int i = blockIdx.x * BX + threadIdx.x + 1, j = blockIdx.y * BY + threadIdx.y + 1, k = blockIdx.z + 1;
  if (i > g.n1 || j > g.n2) return;
  const size_t c = g.ix(i, j, k);
  const real lm = p1d[k - 1] * gar, mm = p1d[g.n3 + k - 1] * gar;
  real vt = s0[c] * lm / mm;
  visct[c] = fmax(vt, 0.);
}
// plane coefficients of the lazy form: cs(k) = max(<LM>/<MM>, 0) for k = 1..n3 (NaN -> 0 as fmax does in k_dsmag_final), ghost planes from
// the z boundary type of the field (periodic: wrap; wall: the neighbour's, the ghost value of |S| carries the sign)
__global__ void k_dsmag_coef(int n3, real gar, const real *__restrict__ p1d, real *__restrict__ cs, int periodic_z) {
  for (int k = threadIdx.x + 1; k <= n3; k += blockDim.x) { const real lm = p1d[k - 1] * gar, mm = p1d[n3 + k - 1] * gar; cs[k] = fmax(lm / mm, 0.); }
  __syncthreads();
  if (threadIdx.x == 0) { cs[0] = periodic_z ? cs[n3] : cs[1]; cs[n3 + 1] = periodic_z ? cs[1] : cs[n3]; }
}
__global__ __launch_bounds__(256) void k_scale_planes(Geom g, const real *__restrict__ cs, real *__restrict__ f) {
  const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
  if (i > g.n1 + 1 || j > g.n2 + 1) return;
  const size_t c = g.ix(i, j, k);
  f[c] = f[c] * cs[k];
}
int materialize_visct(cales_ctx *c) {
  if (!c->visct_lazy) return 0;
  c->visct_lazy = false;
  const int *n = c->n;
  LAUNCH(c, k_scale_planes, dim3((n[0] + 2 + 63) / 64, (n[1] + 2 + 3) / 4, n[2] + 2), dim3(64, 4, 1), 0, c->stream, c->g, c->d_cs, c->f[CALES_VISCT]);
  LAUNCHCHK(c);
  return 0;
}
__global__ __launch_bounds__(256) void k_alph2(Geom g, real w0, real w1, real w2, real w3, real w4, real w5, real *__restrict__ alph2) {
  const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;    // sgs.f90:783-816
  if (i > g.n1 + 1 || j > g.n2 + 1) return;
  const int jg = j + g.jlo;
  const bool near = (w0 != 0. && i == 1) || (w1 != 0. && i == g.n1) || (w2 != 0. && jg == 1) || (w3 != 0. && jg == g.ng2) ||
                    (w4 != 0. && k == 1) || (w5 != 0. && k == g.n3);
  alph2[g.ix(i, j, k)] = near ? 2.52 : 4.00;
}

// ================================================================================================
// Fast path of the dynamic model for cases whose only walls are in z (channels) and without wall model.
// Same arithmetic as the reference sequence (sgs.f90:153-380) re-associated for the hardware, three passes:
//  K_AC  u,v,w -> |S|, |S|Sij, cell-centred velocity, test-filtered velocity        (k_strain_tile / k_corr_strain_tile)
//  K_B + K_DF  filter(|S|Sij) on the fly, filtered velocity, cell-centred velocity -> plane sums of Mij Lij and Mij Mij (k_lmf_tile; the
//        two-pass form k_filter6_tile + k_lij_mij_tile of rounds 1-2 went in round 5)
//  then <LM>/<MM> per plane and visct = max(|S| <LM>/<MM>, 0).
//  * the 27-point top-hat (sgs.f90:632-679) is separable, (1,2,1)^3/64, combined z first, then x, then y;
//  * the wall extrapolation of filtered fields (extrapolate(...,cbc), sgs.f90:705-710,751-766, factor 1) is the rule
//    Q(0) = 2 Q(1) - Q(2) applied to the z combination (filter and extrapolation are linear and commute);
//  * sij, Mij, Lij, LM, MM and the products ui uj are never stored.
// Traffic: ~45 words/cell instead of ~166 measured for the kernel-per-loop sequence (profiles/r01a_*).
// ================================================================================================
// Tile kernels: blocks of 64 x (TY+2) threads march in k; every thread loads its own cell of each input per plane (full
// coalesced rows, next plane prefetched), x neighbours come from DPP lane moves or LDS rows, y neighbours through LDS. The
// kernels that write fields (K_AC, K_B) use tiles of 64 x TY outputs starting at i = 1 + 64 bx so that rows are read and
// written as whole 128-B lines; the read-only K_DF uses 62 x TY outputs with the x halo inside the wave. With the wall rule
// Q(0) = 2Q(1)-Q(2) ghost planes of extrapolated quantities are never read.
__device__ inline void uiuj(const real *s, real *q) {
  q[0] = s[0]; q[1] = s[1]; q[2] = s[2]; q[3] = s[0] * s[0]; q[4] = s[1] * s[1]; q[5] = s[2] * s[2];
  q[6] = s[0] * s[1]; q[7] = s[0] * s[2]; q[8] = s[1] * s[2];
}
struct LijMijArgs {
  const real *uc[3], *uf[3], *mf[6];      // mf[0]: |S| for k_lmf_tile<.., LOCAL> (the layout of this struct is the kernels' argument layout: left as it is)
  real *part;                             // block sums of the planes; k_lmf_tile<.., LOCAL>: visct
  const real *dzci, *dzfi;
  real dxi, dyi;
  int kchunk, nblk, zlo, zhi;
  int wmlo, wmhi; real flo, fhi;      // wall-model z faces: ghost planes of uf,vf by extrapolate(...,lwm), sgs.f90:683-748
  int perx;                             // x ghost columns of uc.., uf.. are not stored: wrap around
  // y walls owned by this rank (k_lmf_tile only): wall rule of the filters along y, alph2 of the wall rows; wall-model y faces: ghost rows of u_f, w_f
  int wylo, wyhi, wmylo, wmyhi;
  // k_lmf_tile<.., UCF = 1>: uc[] are the velocities u, v, w themselves and the cell-centred velocity (sgs.f90:860-869) is formed while loading;
  // vcg = the field whose ghost row 0 holds v_c of the row below the slab (periodic copy or the neighbour's), the one value v(-1) would be needed for
  const real *vcg; int perz, xwrap;      // xwrap: inside cales_step with stale x ghost columns, u(0) is read as u(n1)
};
// K_B + K_D + K_F in one pass (the default): as k_lij_mij_tile, but the test filter of the six products |S|Sij is formed on the fly
// instead of being read back from a pass of its own -- 12 words per cell less (k_filter6_tile's 6 in + 6 out), 12 in and nothing
// but partial sums out. The kernel is bound by its vector instructions (profiles/r02a_sq.md: k_lij_mij_tile VALU busy 0.61, LDS 0.31),
// not by LDS or HBM, and LDS has no room for six more double-buffered filter sums, so the y combination of |S|Sij uses neither:
// every output row loads its own row and the two rows beside it (the neighbours' rows are L1/L2 hits: the same block loads them in
// the same iteration) and combines them in registers; x by DPP, z from two rolling x/y-combined planes. Tiles of 62 x TYL outputs
// with TYL = 8: ten waves per block need <= 168 VGPRs, which holds (without spills in the plane loop) because the 18 loads are issued
// after the register-hungry strain-rate part and folded into six values right after the next barrier; 62 x 6 tiles with eight waves
// measured 4.47 ms against 4.09, variants that spill in the loop 13 ms (profiles/r02d_sq.md: VALU 0.44, waves waiting 0.50).
#ifndef TYL
#define TYL 8
#endif
#ifndef TYLF
#define TYLF 8      // tile height of the instantiations without y walls (their LDS leaves room for twelve rows: six filtered quantities instead of nine)
#endif
#define LMF_TY(YW) ((YW) ? TYL : TYLF)
struct LmfArgs { LijMijArgs L; const real *ss[6]; const real2 *ss2[3]; int by0; BandMap bm; int gx; };      // ss2: |S|Sij as three fields of pairs (PAIR = 1; PAIR = 2: two of pairs, S12 plain at the head of ss2[1]), ss: six fields      // bm: block map of this launch (bm.gx = 0: plain 3-D grid); gx: x tiles of the whole field      // by0: first y tile of this launch (interior and edge tiles of a slab are launched apart)
// Every global access of the plane loop is UNCONDITIONAL (out-of-range lanes, rows and planes are clamped onto valid cells whose values are
// never used): a load inside a divergent branch makes the compiler wait with s_waitcnt vmcnt(0) at the next use of ANY loaded value -- it
// cannot count the operations in flight across the branch -- and that drained, right behind the barrier of every plane, the six loads of
// plane k+2 issued a hundred instructions earlier (HBM latency, once per plane, for all ten waves). With straight-line loads the waits are
// counted: the 18 |S|Sij loads are waited for with the 6 velocity loads of the next plane still in flight, and those with the next 18.
// For the same reason the block sums of a chunk's planes are collected in LDS and stored after the loop (a store inside the loop is a
// vector-memory operation in a branch as well), and the per-plane grid coefficients come through the scalar cache one plane ahead.
constexpr int LMF_KMAX = 256;      // longest k chunk (block sums of a chunk in LDS: 2 x 256 x 8 B of the 9.9 KB the tile leaves)
// UCF = 1: the cell-centred velocity u_c = (u(i) + u(i-1))/2, v_c = (v(j) + v(j-1))/2, w_c = (w(k) + w(k-1))/2 (sgs.f90:860-869, the same expressions
// K_AC stored) is formed here from u, v, w: five loads per plane instead of three, and K_AC writes three fields less (3 of its 16 words; the pass is
// bound by its writes) -- x periodic, z walls or periodic, y periodic / slab neighbours / walls; otherwise UCF = 0 reads the stored fields.
// PAIR = 1: K_AC stored |S|Sij as three fields of PAIRS (S11,S22), (S33,S12), (S13,S23) per cell: nine 16-byte loads per plane instead of eighteen
// 8-byte ones. The pass is bound by what its ten waves issue, not by bytes: 3.95 -> 3.45 ms at 512^3 (K_AC's paired stores cost 0.28 of the 0.5 back).
// PAIR = 2: FIVE components, as k_corr_strain_tile<.., FIVE> left them -- the pairs (S11,S22) in ss2[0] and (S13,S23) in ss2[2], S12 as a plain field at the
// head of ss2[1] -- and |S|S33 not at all: the velocity that pass differenced was the one it had just projected, so S11 + S22 + S33 is the divergence the
// solve left (round-off; chkdiv watches it) and |S|S33 = -(|S|S11 + |S|S22). The test filter with its wall rules is linear: the filtered sixth component is
// the negated sum of the two filtered diagonal ones, formed after the z combination. Fifteen row loads per plane instead of eighteen (six of 16 bytes, three
// of 8), five rolling values per plane instead of six; 11 compulsory words per cell instead of 12. Only inside cales_step (SgsPath::five).
// LOCAL = 1 (SgsAve::local, the reference's _CAVITY, sgs.f90:368-377): nothing is averaged. The pass holds LM and MM of its own cell in registers, so it loads
// |S| of that cell (A.mf[0], one plane ahead, unconditional and clamped like every load of the plane loop) and stores visct = max(|S| LM / MM, 0) of its 62 x TL
// output cells itself (A.part): the partial sums in fours, psum, fold, bsum and the stores of the block sums drop out, and with them k_plane_fold, the
// all-reduce and k_dsmag_final. The store is the one conditional vector-memory operation of the plane loop. MM = 0 gives 0 (fmax(NaN, 0), as in k_dsmag_final).
// Six components only (PAIR = 0 or 1): a cell-wise coefficient has no lazy form, and the plan keeps five components out.
// PACK = 1 (SgsPath::lmf_packed; pair fields on one rank): the REMAINDER x tile of every row -- rem = n1 mod 62 live columns, 16 of 64 lanes at 512 cells, on
// which the unpacked form runs the whole plane loop with 46 lanes clamped onto cells nobody uses. S stretches of rem + 2 lanes, each with its own two halo lanes
// and on a y tile of its own, share a wave, one every P lanes (P = rem + 2 rounded up to a multiple of four, S = 64 / P; lmf_pack.hpp: the map, checked on the
// CPU); the full tiles go in a launch of the unpacked form with grid.x = n1 / 62. The plane loop is the same -- column, row, |S|Sij row and outok per lane come
// from the prologue: lane_prev / lane_next across a stretch's border feed halo lanes only, the LDS neighbours [ty +- 1][tx], [ty][tx - 1] of an output lane stay
// in its stretch, dead stretches (y tiles beyond the last) and dead lanes sit on the last tile's rows and add zero to psum. Block sums: ONE PER STRETCH, formed by
// the operations the unpacked tile's sum takes (stretches start on a multiple of four, so the partials of four are the same; fold adds each stretch's from the
// places they have in the unpacked tile) and stored in the slot the one launch gives that y tile's remainder tile: the plane sums are the one launch's to the bit.
// PAIR = 1 and 2, YW = 0, UCF = 1, 32-bit offsets.
// (PAIR, LOCAL and PACK: one template parameter, SSF = PAIR + 4 LOCAL + 8 PACK, as in k_strain_tile -- the instantiations without LOCAL / PACK keep their symbols.)
// The values of SSF by name. lmf_kernel (below, the one place the instantiations are named) spells them as the literal numbers -- the launch check reports the
// spelled name and the tests match it -- and asserts them against these: 1 pair, 2 pair5, 4 / 5 local without / with pair fields, 9 / 10 packed pair / pair5.
constexpr int LMF_PAIR = 1, LMF_PAIR5 = 2, LMF_LOCAL = 4, LMF_PACK = 8;
template <typename OFF, int YW, int UCF, int SSF = 0>      // YW = 1: walls or wall-model faces in y (ducts); 0: the channel instantiation carries none of that logic
__global__ __launch_bounds__(64 * (LMF_TY(YW) + 2)) void k_lmf_tile(Geom g, LmfArgs B) {
  static constexpr int PAIR = SSF & 3, LOCAL = (SSF >> 2) & 1, PACK = SSF >> 3;      // (static: an automatic constant would join the captures of the lambdas below and shuffle their registers)
  static_assert(PAIR <= 2 && LOCAL <= 1 && (!LOCAL || PAIR != 2), "local averaging keeps six components");
  static_assert(PACK <= 1 && (!PACK || (PAIR && !LOCAL && !YW && UCF)), "the packed remainder tile: pair fields on one rank");
  const LijMijArgs &A = B.L;
  constexpr int TL = LMF_TY(YW);      // tile height
  // FUC (no walls in y): the test-filtered CELL-CENTRED velocity is not filtered here -- the filter is linear and shift-invariant, so F(u_c) =
  // F((u(i) + u(i-1))/2) = (u_f(i) + u_f(i-1))/2, and the filtered face velocity u_f (K_AC's output) is in this pass's LDS ring anyway for the strain rate
  // of the filtered field; likewise v_f along y and w_f along z. Three of the nine quantities leave the z/x/y filter (a third of its LDS traffic, 12 %
  // of the pass's vector instructions). The identity holds wherever the two filters treat the walls alike: everywhere for the tangential components
  // (K_AC extrapolates u, v through a z wall exactly as the wall rule Q(0) = 2Q(1) - Q(2) does), not for w in the two planes next to a z wall, where the
  // reference extrapolates the cell-centred w_c (sgs.f90:751-766) and the face values are what they are: those planes keep the filter of w_c (slot 0).
  constexpr bool FUC = !YW;
  constexpr int NSH = FUC ? 6 : 9, Q0 = FUC ? 3 : 0;      // filtered through LDS: the six products, or all nine
  __shared__ real sh[2][NSH][TL + 2][64];
  __shared__ real shw[FUC ? TL + 2 : 1][64];      // FUC: w_c in the plane next to a z wall (one buffer: the two wall planes are never consecutive, n3 >= 3)
  __shared__ real ring[4][3][TL + 2][64];
  // plane sums: every working wave adds its lanes in fours (two DPP steps) and leaves sixteen partial sums per quantity; the first halo wave, idle
  // behind the barrier, adds the 128 partials of the previous plane (the full six-step wave sum ran in all ten waves before: 24 vector instructions
  // per plane and wave less in a pass that is bound by them)
  __shared__ real psum[LOCAL ? 1 : 2][LOCAL ? 1 : 2][LOCAL ? 1 : TL][16];      // (LOCAL: no sums, see above)
  __shared__ real bsum[LOCAL ? 1 : 2][LOCAL ? 1 : LMF_KMAX];
  const int tx = threadIdx.x, ty = threadIdx.y;
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (!PACK && B.bm.gx && !band_block(B.bm, bx, by, bz)) return;
  by += B.by0;
  // PACK: S stretches of rem + 2 lanes per wave, each on a y tile of its own (lmf_pack.hpp) -- column, row and tile per lane; nothing behind this prologue differs
  const LmfPack pp = PACK ? lmf_pack(g.n1) : LmfPack{};
  const LmfLane pk = PACK ? lmf_pack_lane(pp, tx, ty, (int)blockIdx.y, B.by0, TL, g.n2) : LmfLane{};
  const int nlive = PACK ? min(pp.S, (g.n2 + TL - 1) / TL - ((int)blockIdx.y * pp.S + B.by0)) : 0;      // stretches of this block whose y tile exists
  const int i = PACK ? pk.i : bx * 62 + tx, j = PACK ? pk.j : by * TL + ty;
  const int kbeg = bz * A.kchunk + 1, kend = min(kbeg + A.kchunk - 1, g.n3);
  const bool outok = PACK ? pk.out : tx >= 1 && tx <= 62 && ty >= 1 && ty <= TL && i <= g.n1 && j <= g.n2;
  const int iw = A.perx ? (i == 0 ? g.n1 : (i == g.n1 + 1 ? 1 : i)) : i;
  const int ic = min(iw, g.n1 + 1), jc = min(j, g.n2 + 1);      // clamped: lanes / rows beyond the field read its last ghost column / row
  const OFF c0 = (OFF)g.ix(ic, jc, 0) * RSZ, sk = (OFF)g.s12 * RSZ, sj = (OFF)g.s1 * RSZ;      // byte offsets
  real s0n = 0.;      // LOCAL: |S| of this thread's cell, one plane ahead (an output cell has ic = i, jc = j: c0 is its own column)
  if constexpr (LOCAL) s0n = ldb(A.mf[0], c0 + (OFF)kbeg * sk);
  // rows whose |S|Sij this thread combines: its own and the two beside it; the two halo waves (and rows beyond n2) take a row of the tile
  // interior instead (cache hits, results unused)
  const int jo = PACK ? pk.jo : max(by * TL + 1, min(min(j, by * TL + TL), g.n2));
  const OFF c0s = (OFF)g.ix(ic, jo, 0) * RSZ;
  real sm[3], sc[3], sp[3], sn[3], fn[3];
  // ghost rows of u_f and w_f at wall-model y faces: 2 Q(1) - Q(2) along y (extrapolate(...,lwm) after bounduvw, sgs.f90:683-748); v_f keeps its own.
  // Branch-free: every row loads two values, c1 Q(o1) - c2 Q(o2), with (c1, c2) = (1, 0) and o1 = o2 = its own cell away from such a face
  const int yex = !YW ? 0 : (A.wmylo && j == 0) ? 1 : (A.wmyhi && j == g.n2 + 1) ? -1 : 0;
  const OFF e1 = yex > 0 ? sj : 0, e2 = yex > 0 ? 2 * sj : 0, b1 = yex < 0 ? sj : 0, b2 = yex < 0 ? 2 * sj : 0;      // o + e - b (unsigned offsets: no negative steps)
  const real ec1 = yex != 0 ? 2. : 1., ec2 = yex != 0 ? 1. : 0.;
  auto ldf = [&](int q, OFF o) -> real {
    if (YW && q != 1) return ec1 * ldb(A.uf[q], o + e1 - b1) - ec2 * ldb(A.uf[q], o + e2 - b2);
    return ldb(A.uf[q], o);
  };
  const bool ylo = YW && A.wylo && j == 1, yhi = YW && A.wyhi && j == g.n2;      // rows next to a y wall: ghost row of every filtered quantity = 2 Q(1) - Q(2)
  // UCF: v(j) and v(j-1) of this thread's row, or -- ghost row 0, whose lower neighbour is not in the slab -- the stored v_c of that row with weight 1
  const real *pva = (UCF && jc == 0) ? A.vcg : A.uc[1];
  const OFF ovb = (UCF && jc > 0) ? sj : 0;
  const real cva = (UCF && jc == 0) ? 1. : .5, cvb = (UCF && jc == 0) ? 0. : .5;
  real wprev = 0.;
  const OFF c0m = (OFF)g.ix((A.xwrap && ic == 1) ? g.n1 : max(ic - 1, 0), jc, 0) * RSZ;      // u(i-1): the wrapped column left of the first cell of a row
  auto ucload = [&](int kk, real *o) {      // cell-centred velocity of plane kk (wprev = w of plane kk - 1 on entry, of plane kk on exit)
    const OFF a = c0 + (OFF)kk * sk;
    o[0] = .5 * (ldb(A.uc[0], a) + ldb(A.uc[0], c0m + (OFF)kk * sk));
    o[1] = cva * ldb(pva, a) + cvb * ldb(A.uc[1], a - ovb);
    const real wn = ldb(A.uc[2], a); o[2] = .5 * (wn + wprev); wprev = wn;
  };
  if (UCF) {
    const int k2 = kbeg - 2 >= 0 ? kbeg - 2 : (A.perz ? g.n3 - 1 : 0);      // w below the first plane (periodic z: wrapped; walls: never used)
    wprev = ldb(A.uc[2], c0 + (OFF)k2 * sk);
    ucload(kbeg - 1, sm); ucload(kbeg, sc); ucload(kbeg + 1, sp);
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    if (!UCF) {
      sm[q] = ldb(A.uc[q], c0 + (OFF)(kbeg - 1) * sk);
      sc[q] = ldb(A.uc[q], c0 + (OFF)kbeg * sk);
      sp[q] = ldb(A.uc[q], c0 + (OFF)(kbeg + 1) * sk);
    }
    ring[(kbeg - 1) & 3][q][ty][tx] = ldf(q, c0 + (OFF)(kbeg - 1) * sk);
    ring[kbeg & 3][q][ty][tx] = ldf(q, c0 + (OFF)kbeg * sk);
    fn[q] = ldf(q, c0 + (OFF)(kbeg + 1) * sk);
    if (A.wmlo && kbeg == 1 && q < 2) ring[0][q][ty][tx] = (1. + A.flo) * ring[1][q][ty][tx] - A.flo * fn[q];
  }
  // |S|Sij: y and x combination of one plane (three rows in, lanes beside by DPP)
  auto ssload = [&](int kk, real (*raw)[3]) {
    if (PAIR == 2) {      // slots: S11, S22 | S12 | S13, S23
      const OFF o1 = c0s + (OFF)kk * sk, o = 2 * o1, s2 = 2 * sj;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const char *f = (const char *)B.ss2[2 * q];
        const real2 a = *(const real2 *)(f + (o - s2)), b = *(const real2 *)(f + o), c_ = *(const real2 *)(f + (o + s2));
        raw[3 * q][0] = a.x; raw[3 * q + 1][0] = a.y; raw[3 * q][1] = b.x; raw[3 * q + 1][1] = b.y; raw[3 * q][2] = c_.x; raw[3 * q + 1][2] = c_.y;
      }
      const real *f12 = (const real *)B.ss2[1];
      raw[2][0] = ldb(f12, o1 - sj); raw[2][1] = ldb(f12, o1); raw[2][2] = ldb(f12, o1 + sj);
    } else if (PAIR) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const OFF o = 2 * (c0s + (OFF)kk * sk), s2 = 2 * sj;      // a pair field is twice as wide: byte offsets double
        const real2 a = *(const real2 *)((const char *)B.ss2[q] + (o - s2)), b = *(const real2 *)((const char *)B.ss2[q] + o), c_ = *(const real2 *)((const char *)B.ss2[q] + (o + s2));
        raw[2 * q][0] = a.x; raw[2 * q + 1][0] = a.y; raw[2 * q][1] = b.x; raw[2 * q + 1][1] = b.y; raw[2 * q][2] = c_.x; raw[2 * q + 1][2] = c_.y;
      }
    } else
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const OFF o = c0s + (OFF)kk * sk;
      raw[q][0] = ldb(B.ss[q], o - sj); raw[q][1] = ldb(B.ss[q], o); raw[q][2] = ldb(B.ss[q], o + sj);
    }
  };
  constexpr int NSS = PAIR == 2 ? 5 : 6;      // |S|Sij components that travel
  auto sscomb = [&](const real (*raw)[3], real *X) {
#pragma unroll
    for (int q = 0; q < NSS; ++q) {
      const real Y = (ylo ? 2. * raw[q][1] - raw[q][2] : raw[q][0]) + 2. * raw[q][1] + (yhi ? 2. * raw[q][1] - raw[q][0] : raw[q][2]);
      X[q] = lane_prev(Y) + 2. * Y + lane_next(Y);
    }
  };
  real xm[NSS], xc[NSS], xp[NSS], rw[NSS][3];
  // the ghost plane below a wall is never used (LO planes take 4 xc); it is read all the same when the chunk starts inside the field
  ssload(kbeg - 1, rw); sscomb(rw, xm);
  ssload(kbeg, rw); sscomb(rw, xc);
  ssload(kbeg + 1, rw);
  const int blk = by * B.gx + bx;      // (PACK: a slot per stretch, see the stores at the end)
  auto fold = [&](int k, int b) {      // block sums of plane k by ONE whole wave, fixed order
    const real *p0 = &psum[b][0][0][0], *p1 = &psum[b][LOCAL ? 0 : 1][0][0];      // (LOCAL: never called; the arrays have one element per dimension)
    static_assert(TL * 16 >= 128 && TL * 16 <= 192, "two or three partials per lane");
    constexpr int NP3 = TL * 16 - 128;      // partials beyond the first 128
    if constexpr (PACK) {
      // a sum per stretch, each by the operations the unpacked tile's one sum takes: a stretch starts on a multiple of four lanes, so its partials of four
      // are the unpacked tile's (psum: P / 4 of the sixteen per row, at s P / 4), and the wave adds them from the places they have there, zeros around them
      static_assert(NP3 == 0, "eight rows: two partials per lane");
      const int G = pp.P >> 2, gq = tx & 15;
      for (int s = 0; s < nlive; ++s) {
        const int o = (tx & ~15) + min(s * G + gq, 15);
        const real a = wave_sum_lane63(gq < G ? p0[o] + p0[o + 64] : 0.), bs = wave_sum_lane63(gq < G ? p1[o] + p1[o + 64] : 0.);
        if (tx == 63) { bsum[0][s * A.kchunk + k - kbeg] = a; bsum[1][s * A.kchunk + k - kbeg] = bs; }      // (sgs_setup_launches: S chunks fit)
      }
      return;
    }
    const int t3 = min(tx, NP3 > 0 ? NP3 - 1 : 0) + 128; const real w3 = (NP3 > 0 && tx < NP3) ? 1. : 0.;
    const real a = wave_sum_lane63(NP3 > 0 ? p0[tx] + p0[tx + 64] + w3 * p0[t3] : p0[tx] + p0[tx + 64]),
               bs = wave_sum_lane63(NP3 > 0 ? p1[tx] + p1[tx + 64] + w3 * p1[t3] : p1[tx] + p1[tx + 64]);
    if (tx == 63) { bsum[0][k - kbeg] = a; bsum[LOCAL ? 0 : 1][k - kbeg] = bs; }
  };
  // grid coefficients of the plane, one plane ahead through the scalar cache (uniform: scalar registers)
  real zcm = ldc(A.dzci, kbeg - 1), zcc = ldc(A.dzci, kbeg), zfc = ldc(A.dzfi, kbeg);
  auto plane = [&](const int k, auto lo_c, auto hi_c) {
    constexpr bool LO = decltype(lo_c)::value, HI = decltype(hi_c)::value;
    const int km = (k - 1) & 3, kc = k & 3, kp = (k + 1) & 3, buf = k & 1;
    const OFF idx = c0 + (OFF)min(k + 2, g.n3 + 1) * sk;      // plane k+2 (clamped behind the last ghost plane: loaded again, never used)
    const real zcn = ldc(A.dzci, k + 1), zfn = ldc(A.dzfi, k + 1);
#pragma unroll
    for (int q = 0; q < 3; ++q)
      ring[kp][q][ty][tx] = (HI && A.wmhi && q < 2) ? (1. + A.fhi) * ring[kc][q][ty][tx] - A.fhi * ring[km][q][ty][tx] : fn[q];
    if (UCF) ucload(min(k + 2, g.n3 + 1), sn);
#pragma unroll
    for (int q = 0; q < 3; ++q) { if (!UCF) sn[q] = ldb(A.uc[q], idx); fn[q] = ldf(q, idx); }
    real qm[9], qc[9], qp[9], r[9];
    uiuj(sc, qc);
    if (!LO && !HI) { uiuj(sm, qm); uiuj(sp, qp); }
#pragma unroll
    for (int q = Q0; q < 9; ++q) {
      const real G = (LO || HI) ? 4. * qc[q] : qm[q] + 2. * qc[q] + qp[q];
      r[q] = lane_prev(G) + 2. * G + lane_next(G);
      sh[buf][q - Q0][ty][tx] = r[q];
    }
    if (FUC && (LO || HI)) { const real G = 4. * qc[2]; r[2] = lane_prev(G) + 2. * G + lane_next(G); shw[ty][tx] = r[2]; }      // w_c next to a z wall
    __syncthreads();
    if constexpr (!LOCAL) { if (k > kbeg && ty == 0) fold(k - 1, buf ^ 1); }
    // plane k+1 of |S|Sij: its 18 loads were issued at the end of the previous plane and are folded into six values here, before
    // the register-hungry part; the next 18 are issued after it (keeps the kernel under the 168 VGPRs that ten waves per block need)
    sscomb(rw, xp);
    real lm = 0., mm = 0.;
    if (outok) {
      real F[9];
#pragma unroll
      for (int q = Q0; q < 9; ++q) {
        const real dn = sh[buf][q - Q0][ty - 1][tx], up = sh[buf][q - Q0][ty + 1][tx];
        F[q] = ((ylo ? 2. * r[q] - up : dn) + 2. * r[q] + (yhi ? 2. * r[q] - dn : up)) / 64.;
      }
      if (FUC) {
        F[0] = .5 * (ring[kc][0][ty][tx] + ring[kc][0][ty][tx - 1]); F[1] = .5 * (ring[kc][1][ty][tx] + ring[kc][1][ty - 1][tx]);
        if (LO || HI) F[2] = (shw[ty - 1][tx] + 2. * r[2] + shw[ty + 1][tx]) / 64.;
        else F[2] = .5 * (ring[kc][2][ty][tx] + ring[km][2][ty][tx]);
      }
      const real l0 = F[3] - F[0] * F[0], l1 = F[4] - F[1] * F[1], l2 = F[5] - F[2] * F[2], l3 = F[6] - F[0] * F[1],
                   l4 = F[7] - F[0] * F[2], l5 = F[8] - F[1] * F[2];
      // strain rate of the test-filtered velocity (sgs.f90:571-630). The eight differences of each off-diagonal component telescope
      // pairwise wherever the metric factor is the same (x and y: always; z: not, the grid is stretched), e.g.
      // (u_cpc-u_ccc)+(u_ccc-u_cmc)+(u_mpc-u_mcc)+(u_mcc-u_mmc) = u_cpc-u_cmc+u_mpc-u_mmc: fewer operations and fewer values in flight
      // (this pass is bound by its vector instructions and registers). Same sum in another association: round-off level differences.
#define RU(dk, dj, di) ring[dk][0][ty + (dj)][tx + (di)]
#define RV(dk, dj, di) ring[dk][1][ty + (dj)][tx + (di)]
#define RW(dk, dj, di) ring[dk][2][ty + (dj)][tx + (di)]
      const real dxi = A.dxi, dyi = A.dyi, zc = zcc, zm = zcm;
      real sij[6];
      { const real u_ccc = RU(kc, 0, 0), u_mcc = RU(kc, 0, -1), v_ccc = RV(kc, 0, 0), v_cmc = RV(kc, -1, 0), w_ccc = RW(kc, 0, 0), w_ccm = RW(km, 0, 0);
        sij[0] = (u_ccc - u_mcc) * dxi; sij[1] = (v_ccc - v_cmc) * dyi; sij[2] = (w_ccc - w_ccm) * zfc;
        // s12 = 1/8 [ dyi (u_cpc - u_cmc + u_mpc - u_mmc) + dxi (v_pcc + v_pmc - v_mcc - v_mmc) ]
        const real du = (RU(kc, 1, 0) - RU(kc, -1, 0)) + (RU(kc, 1, -1) - RU(kc, -1, -1));
        const real dv = (RV(kc, 0, 1) - RV(kc, 0, -1)) + (RV(kc, -1, 1) - RV(kc, -1, -1));
        sij[3] = .125 * (du * dyi + dv * dxi);
        // s13 = 1/8 [ zc (u_ccp - u_ccc + u_mcp - u_mcc) + zm (u_ccc - u_ccm + u_mcc - u_mcm) + dxi (w_pcc + w_pcm - w_mcc - w_mcm) ]
        const real up = (RU(kp, 0, 0) - u_ccc) + (RU(kp, 0, -1) - u_mcc), um = (u_ccc - RU(km, 0, 0)) + (u_mcc - RU(km, 0, -1));
        const real dw = (RW(kc, 0, 1) - RW(kc, 0, -1)) + (RW(km, 0, 1) - RW(km, 0, -1));
        sij[4] = .125 * (up * zc + um * zm + dw * dxi);
        // s23 = 1/8 [ zc (v_ccp - v_ccc + v_cmp - v_cmc) + zm (v_ccc - v_ccm + v_cmc - v_cmm) + dyi (w_cpc + w_cpm - w_cmc - w_cmm) ]
        const real vp = (RV(kp, 0, 0) - v_ccc) + (RV(kp, -1, 0) - v_cmc), vm = (v_ccc - RV(km, 0, 0)) + (v_cmc - RV(km, -1, 0));
        const real dw2 = (RW(kc, 1, 0) - RW(kc, -1, 0)) + (RW(km, 1, 0) - RW(km, -1, 0));
        sij[5] = .125 * (vp * zc + vm * zm + dw2 * dyi); }
#undef RU
#undef RV
#undef RW
      const real s0 = sqrt(2. * (sij[0] * sij[0] + sij[1] * sij[1] + sij[2] * sij[2] + 2. * (sij[3] * sij[3] + sij[4] * sij[4] + sij[5] * sij[5])));
      const real a2s0 = (LO || HI || ylo || yhi ? 2.52 : 4.00) * s0;      // alph2: cells next to any wall (sgs.f90:783-816)
      real m[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        auto zc3 = [&](int s) { return (LO || HI) ? 4. * xc[s] : xm[s] + 2. * xc[s] + xp[s]; };      // filter(|S|Sij) * 64
        // (five components: slot of component q, and the third one from the trace after the full 27-point combination)
        const real G = (PAIR == 2 && q == 2) ? -(zc3(0) + zc3(1)) : zc3(PAIR == 2 && q > 2 ? q - 1 : q);
        m[q] = 2. * (G * (1. / 64.) - a2s0 * sij[q]);                             // Mij, sgs.f90:261-272
      }
      lm = m[0] * l0 + m[1] * l1 + m[2] * l2 + (m[3] * l3 + m[4] * l4 + m[5] * l5) * 2.;       // sgs.f90:344-349
      mm = m[0] * m[0] + m[1] * m[1] + m[2] * m[2] + (m[3] * m[3] + m[4] * m[4] + m[5] * m[5]) * 2.;       // sgs.f90:350-355
      if constexpr (LOCAL) { real vt = s0n * lm / mm; stb(A.part, c0 + (OFF)k * sk, fmax(vt, 0.)); }      // sgs.f90:376-377 (the operations of k_dsmag_final in their order)
    }
    ssload(min(k + 2, g.n3 + 1), rw);
    if constexpr (LOCAL) s0n = ldb(A.mf[0], c0 + (OFF)min(k + 1, g.n3 + 1) * sk);      // |S| of plane k+1 (clamped: the ghost plane's value is never used)
    if constexpr (!LOCAL) {
    lm += dpp_f64<0x111>(lm); lm += dpp_f64<0x112>(lm); mm += dpp_f64<0x111>(mm); mm += dpp_f64<0x112>(mm);      // row_shr 1, 2: lanes 3, 7, 11, ... hold four lanes' sum
    if ((tx & 3) == 3 && ty >= 1 && ty <= TL) { psum[buf][0][ty - 1][tx >> 2] = lm; psum[buf][1][ty - 1][tx >> 2] = mm; }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) { sm[q] = sc[q]; sc[q] = sp[q]; sp[q] = sn[q]; }
#pragma unroll
    for (int q = 0; q < NSS; ++q) { xm[q] = xc[q]; xc[q] = xp[q]; }
    zcm = zcc; zcc = zcn; zfc = zfn;
  };
  {
    const std::true_type T; const std::false_type F_;
    int k = kbeg;
    const int klast = (A.zhi && kend == g.n3) ? kend - 1 : kend;
    if (A.zlo && k == 1 && k <= kend) { plane(k, T, F_); ++k; }
    for (; k <= klast; ++k) plane(k, F_, F_);
    if (k <= kend) plane(k, F_, T);
  }
  if constexpr (LOCAL) return;      // (every cell's visct left in the plane loop)
  __syncthreads();
  if (ty == 0 && kend >= kbeg) fold(kend, kend & 1);
  __syncthreads();
  // the chunk's block sums leave in one go
  if constexpr (PACK) {      // every live stretch's into the slot the unpacked launch gives the remainder tile of its y tile (B.gx: x tiles of a row, the remainder one included)
    const int np = kend - kbeg + 1;
    for (int q = ty * 64 + tx; q < 2 * np * nlive; q += 64 * (TL + 2)) {
      const int w = q & 1, kk = (q >> 1) % np, s = (q >> 1) / np, tile = (int)blockIdx.y * pp.S + s + B.by0;
      A.part[(size_t)(w * g.n3 + kbeg + kk - 1) * A.nblk + tile * B.gx + B.gx - 1] = bsum[w][s * A.kchunk + kk];
    }
    return;
  }
  for (int q = ty * 64 + tx; q < 2 * (kend - kbeg + 1); q += 64 * (TL + 2)) {
    const int w = q & 1, kk = q >> 1;
    A.part[(size_t)(w * g.n3 + kbeg + kk - 1) * A.nblk + blk] = bsum[w][kk];
  }
}

// The last pass under the reference's -D_FILTER_2D (SgsPath::filter2d), for the channel class: x periodic, nothing at the y faces, z between two walls or
// periodic -- k_lmf_tile<OFF, 0, 1> with everything the plane filter makes unnecessary taken out, as a kernel of its own so that k_lmf_tile stays as it is.
// Every test filter is (1,2,1)^2/16 of plane k alone (filter2d, sgs.f90:839-847): no z combination and no wall rule for any quantity, so no LO / HI forms of a
// plane, no rolling x/y-combined planes of |S|Sij (twelve registers: the rows of plane k only, loaded one plane ahead and folded behind the barrier), one
// plane of the cell-centred velocity instead of three, alph2 = 2.52 in every cell (sgs.f90:817-821). With nothing extrapolated the identity of FUC, F(u_c) =
// (u_f(i) + u_f(i-1))/2, holds in every plane for all three components: w_f(0) = F(w(0)) next to a wall (both zero) and across a periodic end (both the
// copy). What stays is the ring of three planes of the filtered velocity for its strain rate, with the ghost planes of wall-model z faces extrapolated
// (extrapolate(...,lwm) after bounduvw, sgs.f90:256-260), the plane sums and the rules of k_lmf_tile: unconditional global accesses in the plane loop,
// counted waits, block sums collected in LDS.
template <typename OFF>
__global__ __launch_bounds__(64 * (TYLF + 2)) void k_lmf_plane_tile(Geom g, LmfArgs B) {
  const LijMijArgs &A = B.L;
  constexpr int TL = TYLF;
  __shared__ real sh[2][6][TL + 2][64];      // the six products u_c u_c combined along x, double-buffered (one barrier per plane)
  __shared__ real ring[4][3][TL + 2][64];
  __shared__ real psum[2][2][TL][16];
  __shared__ real bsum[2][LMF_KMAX];
  const int tx = threadIdx.x, ty = threadIdx.y;
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (B.bm.gx && !band_block(B.bm, bx, by, bz)) return;
  by += B.by0;
  const int i = bx * 62 + tx, j = by * TL + ty;
  const int kbeg = bz * A.kchunk + 1, kend = min(kbeg + A.kchunk - 1, g.n3);
  const bool outok = tx >= 1 && tx <= 62 && ty >= 1 && ty <= TL && i <= g.n1 && j <= g.n2;
  const int iw = A.perx ? (i == 0 ? g.n1 : (i == g.n1 + 1 ? 1 : i)) : i;
  const int ic = min(iw, g.n1 + 1), jc = min(j, g.n2 + 1);      // clamped: lanes / rows beyond the field read its last ghost column / row
  const OFF c0 = (OFF)g.ix(ic, jc, 0) * RSZ, sk = (OFF)g.s12 * RSZ, sj = (OFF)g.s1 * RSZ;      // byte offsets
  const int jo = max(by * TL + 1, min(min(j, by * TL + TL), g.n2));      // the row whose |S|Sij this thread combines with the two beside it (k_lmf_tile)
  const OFF c0s = (OFF)g.ix(ic, jo, 0) * RSZ;
  // cell-centred velocity from u, v, w (k_lmf_tile, UCF): v(j) and v(j-1) of this row, or -- ghost row 0 -- the stored v_c of that row with weight 1
  const real *pva = jc == 0 ? A.vcg : A.uc[1];
  const OFF ovb = jc > 0 ? sj : 0;
  const real cva = jc == 0 ? 1. : .5, cvb = jc == 0 ? 0. : .5;
  const OFF c0m = (OFF)g.ix((A.xwrap && ic == 1) ? g.n1 : max(ic - 1, 0), jc, 0) * RSZ;      // u(i-1): the wrapped column left of the first cell of a row
  real wprev = ldb(A.uc[2], c0 + (OFF)(kbeg - 1) * sk);      // w of the plane below (plane 0: the wall's value or the periodic copy)
  auto ucload = [&](int kk, real *o) {      // cell-centred velocity of plane kk (wprev = w of plane kk - 1 on entry, of plane kk on exit)
    const OFF a = c0 + (OFF)kk * sk;
    o[0] = .5 * (ldb(A.uc[0], a) + ldb(A.uc[0], c0m + (OFF)kk * sk));
    o[1] = cva * ldb(pva, a) + cvb * ldb(A.uc[1], a - ovb);
    const real wn = ldb(A.uc[2], a); o[2] = .5 * (wn + wprev); wprev = wn;
  };
  real sc[3], sp[3], sn[3], fn[3];
  ucload(kbeg, sc); ucload(kbeg + 1, sp);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    ring[(kbeg - 1) & 3][q][ty][tx] = ldb(A.uf[q], c0 + (OFF)(kbeg - 1) * sk);
    ring[kbeg & 3][q][ty][tx] = ldb(A.uf[q], c0 + (OFF)kbeg * sk);
    fn[q] = ldb(A.uf[q], c0 + (OFF)(kbeg + 1) * sk);
    if (A.wmlo && kbeg == 1 && q < 2) ring[0][q][ty][tx] = (1. + A.flo) * ring[1][q][ty][tx] - A.flo * fn[q];
  }
  // |S|Sij of one plane: three rows in, combined along y and x (lanes beside by DPP)
  auto ssload = [&](int kk, real (*raw)[3]) {
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const OFF o = c0s + (OFF)kk * sk;
      raw[q][0] = ldb(B.ss[q], o - sj); raw[q][1] = ldb(B.ss[q], o); raw[q][2] = ldb(B.ss[q], o + sj);
    }
  };
  real rw[6][3];
  ssload(kbeg, rw);
  const int blk = by * B.gx + bx;
  auto fold = [&](int k, int b) {      // block sums of plane k by ONE whole wave, fixed order (k_lmf_tile)
    const real *p0 = &psum[b][0][0][0], *p1 = &psum[b][1][0][0];
    static_assert(TL * 16 >= 128 && TL * 16 <= 192, "two or three partials per lane");
    constexpr int NP3 = TL * 16 - 128;      // partials beyond the first 128
    const int t3 = min(tx, NP3 > 0 ? NP3 - 1 : 0) + 128; const real w3 = (NP3 > 0 && tx < NP3) ? 1. : 0.;
    const real a = wave_sum_lane63(NP3 > 0 ? p0[tx] + p0[tx + 64] + w3 * p0[t3] : p0[tx] + p0[tx + 64]),
               bs = wave_sum_lane63(NP3 > 0 ? p1[tx] + p1[tx + 64] + w3 * p1[t3] : p1[tx] + p1[tx + 64]);
    if (tx == 63) { bsum[0][k - kbeg] = a; bsum[1][k - kbeg] = bs; }
  };
  real zcm = ldc(A.dzci, kbeg - 1), zcc = ldc(A.dzci, kbeg), zfc = ldc(A.dzfi, kbeg);
  auto plane = [&](const int k, auto hi_c) {
    constexpr bool HI = decltype(hi_c)::value;      // the plane below a wall-model top face: its ghost plane is extrapolated into the ring
    const int km = (k - 1) & 3, kc = k & 3, kp = (k + 1) & 3, buf = k & 1;
    const OFF idx = c0 + (OFF)min(k + 2, g.n3 + 1) * sk;      // plane k+2 (clamped behind the last ghost plane: loaded again, never used)
    const real zcn = ldc(A.dzci, k + 1), zfn = ldc(A.dzfi, k + 1);
#pragma unroll
    for (int q = 0; q < 3; ++q)
      ring[kp][q][ty][tx] = (HI && A.wmhi && q < 2) ? (1. + A.fhi) * ring[kc][q][ty][tx] - A.fhi * ring[km][q][ty][tx] : fn[q];
    ucload(min(k + 2, g.n3 + 1), sn);
#pragma unroll
    for (int q = 0; q < 3; ++q) fn[q] = ldb(A.uf[q], idx);
    const real pr[6] = {sc[0] * sc[0], sc[1] * sc[1], sc[2] * sc[2], sc[0] * sc[1], sc[0] * sc[2], sc[1] * sc[2]};      // sgs.f90:283-295
    real r[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) { r[q] = lane_prev(pr[q]) + 2. * pr[q] + lane_next(pr[q]); sh[buf][q][ty][tx] = r[q]; }
    __syncthreads();
    if (k > kbeg && ty == 0) fold(k - 1, buf ^ 1);
    real xc[6];      // filter(|S|Sij) * 16 of plane k: its 18 loads were issued at the end of the previous plane
#pragma unroll
    for (int q = 0; q < 6; ++q) { const real Y = rw[q][0] + 2. * rw[q][1] + rw[q][2]; xc[q] = lane_prev(Y) + 2. * Y + lane_next(Y); }
    real lm = 0., mm = 0.;
    if (outok) {
      real L[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) L[q] = (sh[buf][q][ty - 1][tx] + 2. * r[q] + sh[buf][q][ty + 1][tx]) / 16.;
      const real F0 = .5 * (ring[kc][0][ty][tx] + ring[kc][0][ty][tx - 1]), F1 = .5 * (ring[kc][1][ty][tx] + ring[kc][1][ty - 1][tx]),
                   F2 = .5 * (ring[kc][2][ty][tx] + ring[km][2][ty][tx]);
      const real l0 = L[0] - F0 * F0, l1 = L[1] - F1 * F1, l2 = L[2] - F2 * F2, l3 = L[3] - F0 * F1, l4 = L[4] - F0 * F2, l5 = L[5] - F1 * F2;
      // strain rate of the test-filtered velocity (sgs.f90:571-630), the differences telescoped as in k_lmf_tile
#define RU(dk, dj, di) ring[dk][0][ty + (dj)][tx + (di)]
#define RV(dk, dj, di) ring[dk][1][ty + (dj)][tx + (di)]
#define RW(dk, dj, di) ring[dk][2][ty + (dj)][tx + (di)]
      const real dxi = A.dxi, dyi = A.dyi, zc = zcc, zm = zcm;
      real sij[6];
      { const real u_ccc = RU(kc, 0, 0), u_mcc = RU(kc, 0, -1), v_ccc = RV(kc, 0, 0), v_cmc = RV(kc, -1, 0), w_ccc = RW(kc, 0, 0), w_ccm = RW(km, 0, 0);
        sij[0] = (u_ccc - u_mcc) * dxi; sij[1] = (v_ccc - v_cmc) * dyi; sij[2] = (w_ccc - w_ccm) * zfc;
        const real du = (RU(kc, 1, 0) - RU(kc, -1, 0)) + (RU(kc, 1, -1) - RU(kc, -1, -1));
        const real dv = (RV(kc, 0, 1) - RV(kc, 0, -1)) + (RV(kc, -1, 1) - RV(kc, -1, -1));
        sij[3] = .125 * (du * dyi + dv * dxi);
        const real up = (RU(kp, 0, 0) - u_ccc) + (RU(kp, 0, -1) - u_mcc), um = (u_ccc - RU(km, 0, 0)) + (u_mcc - RU(km, 0, -1));
        const real dw = (RW(kc, 0, 1) - RW(kc, 0, -1)) + (RW(km, 0, 1) - RW(km, 0, -1));
        sij[4] = .125 * (up * zc + um * zm + dw * dxi);
        const real vp = (RV(kp, 0, 0) - v_ccc) + (RV(kp, -1, 0) - v_cmc), vm = (v_ccc - RV(km, 0, 0)) + (v_cmc - RV(km, -1, 0));
        const real dw2 = (RW(kc, 1, 0) - RW(kc, -1, 0)) + (RW(km, 1, 0) - RW(km, -1, 0));
        sij[5] = .125 * (vp * zc + vm * zm + dw2 * dyi); }
#undef RU
#undef RV
#undef RW
      const real s0 = sqrt(2. * (sij[0] * sij[0] + sij[1] * sij[1] + sij[2] * sij[2] + 2. * (sij[3] * sij[3] + sij[4] * sij[4] + sij[5] * sij[5])));
      const real a2s0 = 2.52 * s0;      // alph2 of the -D_FILTER_2D build (sgs.f90:817-821)
      real m[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) m[q] = 2. * (xc[q] * (1. / 16.) - a2s0 * sij[q]);      // Mij, sgs.f90:261-272
      lm = m[0] * l0 + m[1] * l1 + m[2] * l2 + (m[3] * l3 + m[4] * l4 + m[5] * l5) * 2.;       // sgs.f90:344-349
      mm = m[0] * m[0] + m[1] * m[1] + m[2] * m[2] + (m[3] * m[3] + m[4] * m[4] + m[5] * m[5]) * 2.;       // sgs.f90:350-355
    }
    ssload(min(k + 1, g.n3 + 1), rw);
    lm += dpp_f64<0x111>(lm); lm += dpp_f64<0x112>(lm); mm += dpp_f64<0x111>(mm); mm += dpp_f64<0x112>(mm);      // row_shr 1, 2: lanes 3, 7, 11, ... hold four lanes' sum
    if ((tx & 3) == 3 && ty >= 1 && ty <= TL) { psum[buf][0][ty - 1][tx >> 2] = lm; psum[buf][1][ty - 1][tx >> 2] = mm; }
#pragma unroll
    for (int q = 0; q < 3; ++q) { sc[q] = sp[q]; sp[q] = sn[q]; }
    zcm = zcc; zcc = zcn; zfc = zfn;
  };
  {
    const std::true_type T; const std::false_type F_;
    int k = kbeg;
    const int klast = (A.zhi && kend == g.n3) ? kend - 1 : kend;
    for (; k <= klast; ++k) plane(k, F_);
    if (k <= kend) plane(k, T);
  }
  __syncthreads();
  if (ty == 0 && kend >= kbeg) fold(kend, kend & 1);
  __syncthreads();
  // the chunk's block sums leave in one go
  for (int q = ty * 64 + tx; q < 2 * (kend - kbeg + 1); q += 64 * (TL + 2)) {
    const int w = q & 1, kk = q >> 1;
    A.part[(size_t)(w * g.n3 + kbeg + kk - 1) * A.nblk + blk] = bsum[w][kk];
  }
}

// K_A + K_C in one pass over u,v,w: strain rate (sgs.f90:571-630) stored as |S| and |S|Sij, cell-centred velocity (sgs.f90:860-869) and the
// test-filtered velocity (sgs.f90:632-679 with the wall rule), all from an LDS ring of three raw planes.
#ifndef TYS
#define TYS 14      // measured at 512^3 (A/B on one box): 14 beats 6 and 10 for the dynamic-model pass (-7 %) and the Smagorinsky pass (-26 %)
#endif
#ifndef TYC
#define TYC 10      // tile height of k_corr_strain_tile (K_AC with the projection folded in). Measured at 512^3 on one box: 10 rows (twelve waves, 144 VGPRs, 88 KB)
#endif              // 3.37 ms per call, 14 rows (sixteen waves at the 128-register cap, 117 KB) 3.49; a 14-row build that spilled fourteen registers 4.5
struct StrainTileArgs {
  const real *u[3];
  real *s0, *ssij[6], *uc[3], *uf[3];
  real2 *ss2[3];      // PAIR = 1: |S|Sij as three fields of pairs (S11,S22), (S33,S12), (S13,S23) instead of ssij
  const real *dzci, *dzfi;
  real dxi, dyi;
  int kchunk, zlo, zhi;
  int wmlo, wmhi; real flo, fhi;      // wall-model z faces: ghost planes of u,v by extrapolate(...,lwm), sgs.f90:683-748
  // SMAG = 1 (static Smagorinsky with van Driest damping for z walls, sgs.f90:98-152): the only output is visct
  real *visct; const real *zc, *del; real l3, visc;      // del(k) = (dx dy dzf(k))^(1/3)
  // SMAG = 1 with walls in y (ducts): wylo/wyhi = no-slip y walls owned by this rank (van Driest distance and shear, the latter from
  // twy(side, k, i) = sqrt(tau_w) of k_wall_shear_y); wmylo/wmyhi = wall-model y faces: the strain rate sees ghost rows of u and w
  // extrapolated from the interior (extrapolate(...,lwm) along y, sgs.f90:683-748)
  int wylo, wyhi, wmylo, wmyhi; const real *twy; real dl2;
  BandMap bm;      // block -> (x tile, y tile, k chunk) map of the 1-D launches (bm.gx = 0: plain 3-D grid)
  int perx;        // x periodic: halo columns beyond the ends of a row are the wrapped interior columns (the ghost columns may be stale inside cales_step)
  // CORR = 1 (cales_step, x and y periodic, one rank, z walls or z periodic, explicit diffusion, no wall model): u[] is the PREDICTION u*, v*, w* and the
  // projection (correc.f90:44-67 with the deferred bulk forcing) + pressure update (updatep.f90:30-47) happen here -- every velocity value the pass
  // reads is corrected while it is loaded, u = (u* + f) - dtrk grad(pp) at the periodically wrapped interior cell, the z ghost planes by their
  // boundary rule (bounduvw with is_correc, bound.f90:18-154), the corrected velocity of the tile's own cells goes to un[] (a second set of buffers:
  // neighbouring tiles still read u*) and p += pp in place. The pass k_correc_cell<1> (9 words per cell) disappears: 13 + 9 -> 19 words.
  const real *pp; real *p; real *un[3]; const real *force; int fmask; real cfi, cfj, cdt;
  real *vcg = nullptr;      // EXT = 1: the field whose ghost rows 0 and n2+1 receive v_c (LijMijArgs::vcg)
  const real *bcz[2][2];      // Dirichlet planes of u and v at the two z walls (bounduvw's 2 bc - u(1)), [component][side]
  int zper;                   // z periodic: ghost planes are the wrapped interior planes
  // several slabs (pery = 0): the ghost rows 0 and n2+1 of u*, v*, w* and pp hold the neighbours' rows (exchanged), and the one value further out that the
  // correction of v in row n2+1 needs -- pp of the upper neighbour's row 2 -- sits in ghost row n2+1 of the COMPANION field, allocated right behind pp
  // (ppd = its distance in bytes; cales_step copies row 2 there and exchanges both fields in one message). One slab: rows wrap around.
  int pery; size_t ppd;
};
// sqrt(tau_w) at the two y walls for every (i, k): the argument of the van Driest damping of the cells whose nearest wall is a y wall
// (sgs.f90:117-143, cases 3 and 4 of the select), from the fields themselves (their ghost cells, not the extrapolated ones)
__global__ __launch_bounds__(256) void k_wall_shear_y(Geom g, const real *__restrict__ u, const real *__restrict__ w, real visc, real dyi,
                                                      int lo, int hi, real *__restrict__ twy, int perx) {
  const int i = blockIdx.x * 64 + threadIdx.x + 1, k = blockIdx.y * 4 + threadIdx.y + 1;
  if (i > g.n1 || k > g.n3) return;
  const int n2 = g.n2;
  const int im1 = (perx && i == 1) ? g.n1 : i - 1;      // x periodic inside cales_step: the wrapped interior column, the ghost column 0 may be stale (step_xskip)
  if (lo) {
    const real t1 = u[g.ix(i, 1, k)] - u[g.ix(i, 0, k)] + u[g.ix(im1, 1, k)] - u[g.ix(im1, 0, k)];
    const real t2 = w[g.ix(i, 1, k)] - w[g.ix(i, 0, k)] + w[g.ix(i, 1, k - 1)] - w[g.ix(i, 0, k - 1)];
    twy[(size_t)k * g.s1 + i] = sqrt(0.5 * visc * (sqrt(t1 * t1 + t2 * t2) * dyi));
  }
  if (hi) {
    const real t1 = u[g.ix(i, n2, k)] - u[g.ix(i, n2 + 1, k)] + u[g.ix(im1, n2, k)] - u[g.ix(im1, n2 + 1, k)];
    const real t2 = w[g.ix(i, n2, k)] - w[g.ix(i, n2 + 1, k)] + w[g.ix(i, n2, k - 1)] - w[g.ix(i, n2 + 1, k - 1)];
    twy[(size_t)(g.n3 + 2 + k) * g.s1 + i] = sqrt(0.5 * visc * (sqrt(t1 * t1 + t2 * t2) * dyi));
  }
}
// F2D = 1 (the reference's -D_FILTER_2D): the filtered velocity is the in-plane (1,2,1)^2/16 of plane k of the raw u, v, w (filter2d, sgs.f90:244-246,839-847):
// no z combination, no wall rule; the strain rate and the wall-model ghost planes of the ring are what they were
// (PAIR and F2D: the values 1 and 2 of one template parameter, as in k_lmf_tile.)
constexpr int STRAIN_PAIR = 1, STRAIN_F2D = 2;      // the values of SSF by name (strain_kernel below spells them as numbers, as lmf_kernel does)
template <typename OFF, int TY, int YW, int SSF = 0>      // YW = 1: walls or wall-model faces in y (ducts); the channel instantiations carry none of that logic
__global__ __launch_bounds__(64 * (TY + 2)) void k_strain_tile(Geom g, StrainTileArgs A) {
  constexpr int PAIR = SSF == 1, F2D = SSF == 2;
  static_assert(!F2D || (!YW && !PAIR), "the plane filter is built for the channel class");
  // (one barrier per plane with four ring slots and double-buffered sums, as in k_lij_mij_tile, measured 13 % slower here)
  __shared__ real ring[3][3][TY + 2][66];      // rows: x-halo cell, 64 own cells, x-halo cell
  __shared__ real shs[3][TY + 2][64];
  const int tx = threadIdx.x, ty = threadIdx.y;
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (A.bm.gx && !band_block(A.bm, bx, by, bz)) return;
  const int i = bx * 64 + tx + 1, j = by * TY + ty;        // whole 128-B lines in and out (see cales_create)
  const int kbeg = bz * A.kchunk + 1, kend = min(kbeg + A.kchunk - 1, g.n3);
  const bool edge = tx == 0 || tx == 63;
  const int ih0 = tx == 0 ? i - 1 : i + 1, hx = tx == 0 ? 0 : 65;
  const int ih = !A.perx ? ih0 : ih0 == 0 ? g.n1 : ih0 == g.n1 + 1 ? 1 : ih0;
  const bool ldok = i <= g.n1 + 1 && j <= g.n2 + 1, hok = edge && ih0 <= g.n1 + 1 && j <= g.n2 + 1;
  const bool outok = ty >= 1 && ty <= TY && i <= g.n1 && j <= g.n2;
  const int iq = (A.perx && i == g.n1 + 1) ? 1 : i;      // (the column right of the last cell of the row, loaded by the last tile's lane beside it)
  const OFF c0 = ldok ? (OFF)g.ix(iq, j, 0) * RSZ : 0, ch = hok ? (OFF)g.ix(ih, j, 0) * RSZ : 0, sk = (OFF)g.s12 * RSZ;   // byte offsets
  real fn[3], fh[3];
  // ghost rows at wall-model y faces: u and w are replaced by 2 Q(1) - Q(2) along y; v, normal to the face, is not
  const int yex = !YW ? 0 : (A.wmylo && j == 0) ? 1 : (A.wmyhi && j == g.n2 + 1) ? -1 : 0;
  const OFF sjb = (OFF)g.s1 * RSZ;
  auto ld = [&](int q, OFF o) -> real {
    if (YW && yex != 0 && q != 1) return yex > 0 ? 2. * ldb(A.u[q], o + sjb) - ldb(A.u[q], o + 2 * sjb) : 2. * ldb(A.u[q], o - sjb) - ldb(A.u[q], o - 2 * sjb);
    return ldb(A.u[q], o);
  };
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    ring[(kbeg - 1) % 3][q][ty][tx + 1] = ldok ? ld(q, c0 + (OFF)(kbeg - 1) * sk) : 0.;
    ring[kbeg % 3][q][ty][tx + 1] = ldok ? ld(q, c0 + (OFF)kbeg * sk) : 0.;
    if (edge) {
      ring[(kbeg - 1) % 3][q][ty][hx] = hok ? ld(q, ch + (OFF)(kbeg - 1) * sk) : 0.;
      ring[kbeg % 3][q][ty][hx] = hok ? ld(q, ch + (OFF)kbeg * sk) : 0.;
    }
    fn[q] = ldok ? ld(q, c0 + (OFF)(kbeg + 1) * sk) : 0.;
    fh[q] = hok ? ld(q, ch + (OFF)(kbeg + 1) * sk) : 0.;
    if (A.wmlo && kbeg == 1 && q < 2) {
      ring[0][q][ty][tx + 1] = (1. + A.flo) * ring[1][q][ty][tx + 1] - A.flo * fn[q];
      if (edge) ring[0][q][ty][hx] = (1. + A.flo) * ring[1][q][ty][hx] - A.flo * fh[q];
    }
  }
  int km = (kbeg - 1) % 3, kc = kbeg % 3, kp = (kbeg + 1) % 3;
  for (int k = kbeg; k <= kend; ++k) {
    const OFF idx = c0 + (OFF)k * sk;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const bool ex = A.wmhi && k == g.n3 && q < 2;
      ring[kp][q][ty][tx + 1] = ex ? (1. + A.fhi) * ring[kc][q][ty][tx + 1] - A.fhi * ring[km][q][ty][tx + 1] : fn[q];
      if (edge) ring[kp][q][ty][hx] = ex ? (1. + A.fhi) * ring[kc][q][ty][hx] - A.fhi * ring[km][q][ty][hx] : fh[q];
    }
    if (k + 2 <= g.n3 + 1) {
#pragma unroll
      for (int q = 0; q < 3; ++q) { fn[q] = ldok ? ld(q, idx + 2 * sk) : 0.; fh[q] = hok ? ld(q, ch + (OFF)(k + 2) * sk) : 0.; }
    }
    __syncthreads();
    const bool lo = A.zlo && k == 1, hi = A.zhi && k == g.n3;
    real r[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      auto zcomb = [&](int x) {
        const real qm = ring[km][q][ty][x], qc = ring[kc][q][ty][x], qp = ring[kp][q][ty][x];
        const real vm = (lo && q < 2) ? 2. * qc - qp : qm;      // u,v extrapolated through the walls, w (on the faces) not
        const real vp = (hi && q < 2) ? 2. * qc - qm : qp;
        return vm + 2. * qc + vp;
      };
      const real G = F2D ? ring[kc][q][ty][tx + 1] : zcomb(tx + 1);
      real pv = lane_prev(G), nx = lane_next(G);
      if (edge) { const real Gh = F2D ? ring[kc][q][ty][hx] : zcomb(hx); if (tx == 0) pv = Gh; else nx = Gh; }
      r[q] = pv + 2. * G + nx;
      shs[q][ty][tx] = r[q];
    }
    if (outok) {
#define RU(dk, dj, di) ring[dk][0][ty + (dj)][tx + 1 + (di)]
#define RV(dk, dj, di) ring[dk][1][ty + (dj)][tx + 1 + (di)]
#define RW(dk, dj, di) ring[dk][2][ty + (dj)][tx + 1 + (di)]
      const real u_mcm = RU(km, 0, -1), u_ccm = RU(km, 0, 0), u_mmc = RU(kc, -1, -1), u_cmc = RU(kc, -1, 0), u_mcc = RU(kc, 0, -1),
                   u_ccc = RU(kc, 0, 0), u_mpc = RU(kc, 1, -1), u_cpc = RU(kc, 1, 0), u_mcp = RU(kp, 0, -1), u_ccp = RU(kp, 0, 0);
      const real v_cmm = RV(km, -1, 0), v_ccm = RV(km, 0, 0), v_mmc = RV(kc, -1, -1), v_cmc = RV(kc, -1, 0), v_pmc = RV(kc, -1, 1),
                   v_mcc = RV(kc, 0, -1), v_ccc = RV(kc, 0, 0), v_pcc = RV(kc, 0, 1), v_cmp = RV(kp, -1, 0), v_ccp = RV(kp, 0, 0);
      const real w_cmm = RW(km, -1, 0), w_mcm = RW(km, 0, -1), w_ccm = RW(km, 0, 0), w_pcm = RW(km, 0, 1), w_cpm = RW(km, 1, 0),
                   w_cmc = RW(kc, -1, 0), w_mcc = RW(kc, 0, -1), w_ccc = RW(kc, 0, 0), w_pcc = RW(kc, 0, 1), w_cpc = RW(kc, 1, 0);
#undef RU
#undef RV
#undef RW
      const real dxi = A.dxi, dyi = A.dyi, zc = ldc(A.dzci, k), zm = ldc(A.dzci, k - 1);
      const real s11 = (u_ccc - u_mcc) * dxi, s22 = (v_ccc - v_cmc) * dyi, s33 = (w_ccc - w_ccm) * ldc(A.dzfi, k);
      const real s12 = .125 * ((u_cpc - u_ccc) * dyi + (v_pcc - v_ccc) * dxi + (u_ccc - u_cmc) * dyi + (v_pmc - v_cmc) * dxi +
                                 (u_mpc - u_mcc) * dyi + (v_ccc - v_mcc) * dxi + (u_mcc - u_mmc) * dyi + (v_cmc - v_mmc) * dxi);
      const real s13 = .125 * ((u_ccp - u_ccc) * zc + (w_pcc - w_ccc) * dxi + (u_ccc - u_ccm) * zm + (w_pcm - w_ccm) * dxi +
                                 (u_mcp - u_mcc) * zc + (w_ccc - w_mcc) * dxi + (u_mcc - u_mcm) * zm + (w_ccm - w_mcm) * dxi);
      const real s23 = .125 * ((v_ccp - v_ccc) * zc + (w_cpc - w_ccc) * dyi + (v_ccc - v_ccm) * zm + (w_cpm - w_ccm) * dyi +
                                 (v_cmp - v_cmc) * zc + (w_ccc - w_cmc) * dyi + (v_cmc - v_cmm) * zm + (w_ccm - w_cmm) * dyi);
      const real s0v = sqrt(2. * (s11 * s11 + s22 * s22 + s33 * s33 + 2. * (s12 * s12 + s13 * s13 + s23 * s23)));
      {
        stb(A.s0, idx, s0v);                                              // stands for visct = s0 (sgs.f90:184) until the final kernel
        if (PAIR) {      // |S|Sij (sgs.f90:198-210), two components per 16-byte store
          const OFF i2 = 2 * idx;
          typedef real v2 __attribute__((ext_vector_type(2)));      // (streaming stores: -2 % on this pass, measured three times)
          __builtin_nontemporal_store(v2{s0v * s11, s0v * s22}, (v2 *)((char *)A.ss2[0] + i2));
          __builtin_nontemporal_store(v2{s0v * s33, s0v * s12}, (v2 *)((char *)A.ss2[1] + i2));
          __builtin_nontemporal_store(v2{s0v * s13, s0v * s23}, (v2 *)((char *)A.ss2[2] + i2));
        } else {
        stb(A.ssij[0], idx, s0v * s11); stb(A.ssij[1], idx, s0v * s22); stb(A.ssij[2], idx, s0v * s33);      // |S|Sij (sgs.f90:198-210)
        stb(A.ssij[3], idx, s0v * s12); stb(A.ssij[4], idx, s0v * s13); stb(A.ssij[5], idx, s0v * s23);
        }
        if (A.uc[0]) { stb(A.uc[0], idx, 0.5 * (u_ccc + u_mcc)); stb(A.uc[1], idx, 0.5 * (v_ccc + v_cmc)); stb(A.uc[2], idx, 0.5 * (w_ccc + w_ccm)); }      // (null: the last pass forms them itself)
      }
    }
    __syncthreads();
    if (outok) {
      // next to a no-slip y wall the ghost row of u and w is the extrapolation 2 Q(1) - Q(2) (extrapolate(...,cbc), sgs.f90:705-710): its
      // y combination is 4 Q(1); v, normal to the wall, keeps its ghost row
      const bool ylo = YW && A.wylo && j == 1, yhi = YW && A.wyhi && j == g.n2;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const real dn = shs[q][ty - 1][tx], up = shs[q][ty + 1][tx];
        const real a = (ylo && q != 1) ? 2. * r[q] - up : dn, b = (yhi && q != 1) ? 2. * r[q] - dn : up;
        stb(A.uf[q], idx, (a + 2. * r[q] + b) / (F2D ? 16. : 64.));
      }
    }
    const int t = km; km = kc; kc = kp; kp = t;
  }
}
// ---- K_AC with the projection folded in (StrainTileArgs, "CORR"; cales_step on one rank, x and y periodic, z walls or periodic): every velocity value
// the pass reads is corrected while it is loaded, u = (u* + f) - dtrk grad(pp) at the periodically wrapped interior cell (the operations of
// k_correc_cell in their order), the z ghost planes by their boundary rule; the corrected velocity of the tile's own cells goes to un[] (a second set of
// buffers: neighbouring tiles still read u*) and p += pp in place. Same tile, ring and strain-rate / filter arithmetic as k_strain_tile<.., PAIR = 1>.
// Memory accesses are laid out for the hardware's in-order counters (see k_momrk): every global access of the plane loop is unconditional straight-line
// code -- loads from clamped / wrapped cells, stores of lanes without an output to the x ghost cell of their row (dead inside cales_step: every reader
// wraps around, the step's last ghost-cell update rewrites it) -- so the waits are counted (the loads of plane k+2 stay in flight behind the eleven
// stores of plane k) instead of s_waitcnt vmcnt(0) at every use. A plane is completed ONE iteration after its loads were issued. The two y-halo
// waves have no outputs: they run a loop of their own and complete the tile's two x-halo COLUMNS, one tile row per lane (wave 0 the column left of the
// tile, wave TY+1 the one right of it), which as a branch of the edge lanes ran in every one of the sixteen waves.
// EXT = 1 (several slabs, StepPlan::fold_rows2): the tile rows start one row lower and the pass ALSO forms the two ghost rows j = 0 and n2+1 of everything
// it writes -- corrected u, v, w, p + pp, |S|, |S|Sij, the filtered velocity, and v_c of those two rows for the last pass (A.vcg) -- from a SECOND ghost
// row of the prediction (rows -1 / n2+2: the ghost rows 0 / n2+1 of the companion field that sits A.ppd bytes behind every velocity field) and a third of
// pp (row n2+3: its second companion): nothing this pass produces travels between the slabs afterwards.
// FIVE (one rank, SgsPath::five): |S|S33 is not stored -- S11 + S22 + S33 is the divergence of the velocity this very pass has projected, round-off of the
// solve, so the last pass takes |S|S33 = -(|S|S11 + |S|S22) (k_lmf_tile, PAIR = 2) -- and |S|S12, left without a partner, goes as a plain field to the head of
// ss2[1]: 13 words written per cell instead of 14, 18 words in all instead of 19. |S| itself is formed from the true S33, in registers, as before. Valid only
// HERE: cmpt_sgs outside the step (start-up, operator-level calls) sees a velocity nobody has projected and keeps six components.
// (EXT and FIVE: the values 1 and 2 of one template parameter, as in k_strain_tile -- slabs keep six components.)
template <typename OFF, int TY, int ROWS = 0>
__global__ __launch_bounds__(64 * (TY + 2)) void k_corr_strain_tile(Geom g, StrainTileArgs A) {
  constexpr int EXT = ROWS == 1, FIVE = ROWS == 2;
  __shared__ real ring[3][3][TY + 2][66];      // rows: x-halo cell, 64 own cells, x-halo cell
  __shared__ real shs[3][TY + 2][64];
  // pp of the tile's cells, planes k+1 / k+2 (by parity), column 64 = the x-halo cell right of the row: the correction of a cell needs pp(i+1) (the lane
  // beside: DPP; last lane: column 64), pp(j+1) (the row above: here) and pp(k+1) (its own next value) -- two global loads per cell and plane less
  __shared__ real sP[2][TY + 2][65];
  const int tx = threadIdx.x, ty = threadIdx.y;
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (A.bm.gx && !band_block(A.bm, bx, by, bz)) return;
  const int n1 = g.n1, n2 = g.n2, n3 = g.n3;      // (n1 a multiple of 64: every tile is full in x, dsmag_fast)
  const int i = bx * 64 + tx + 1, j = by * TY + ty - EXT;
  const int kbeg = bz * A.kchunk + 1, kend = min(kbeg + A.kchunk - 1, n3);
  const bool edge = tx == 0 || tx == 63;
  const int hx = tx == 0 ? 0 : 65;
  const bool outok = ty >= 1 && ty <= TY && j >= 1 - EXT && j <= n2 + EXT;
  // the rows this thread loads. One slab: wrapped in y (rows beyond n2+1 keep wrapping: row n2+2 holds pp of row 2, which the correction of row n2+1 --
  // the wrapped row 1, the halo of the last row -- reads from sP). Several slabs: the ghost rows as they are, pp of "row n2+2" from the companion field
  auto urow = [&](int r) { return A.pery ? (r == 0 ? n2 : r > n2 ? min(r - n2, n2) : r) : min(max(r, 0), n2 + 1); };
  // byte offset (from its field's base) of cell (col, row r, plane 0) of a field with `nc` companions behind it: several slabs -- the rows 0 .. n2+1 as they
  // are, row -1 in the first companion's ghost row 0, row n2+1+q (q = 1 .. nc) in companion q's ghost row n2+1 (rows further out: the last of them; the
  // values only reach tile rows that have no output). nc = 0: clamped to the ghost rows.
  auto foff = [&](int col, int r, int nc) -> OFF {
    if (A.pery) return (OFF)g.ix(col, urow(r), 0) * RSZ;
    if (EXT && r < 0) return (OFF)(A.ppd + g.ix(col, 0, 0) * RSZ);
    if (r <= n2 + 1 || nc == 0) return (OFF)g.ix(col, min(r, n2 + 1), 0) * RSZ;
    return (OFF)((size_t)min(r - (n2 + 1), nc) * A.ppd + g.ix(col, n2 + 1, 0) * RSZ);
  };
  constexpr int NCV = EXT, NCP = 1 + EXT;      // companions of the velocity fields / of pp
  const int jq = urow(j);
  const OFF sk = (OFF)g.s12 * RSZ;
  const OFF cl = foff(i, j, NCV), clp = foff(i, j, NCP), cly = foff(i, j + 1, NCP);
  const OFF cdump = (OFF)g.ix(0, min(max(j, 0), n2 + 1), 0) * RSZ;      // the x ghost cell of the row: where lanes / planes without an output of their own store
  const OFF cst = outok ? cl : cdump;
  const OFF cvc = (EXT && outok && (j == 0 || j == n2 + 1)) ? cl : cdump;
  // side job of the y-halo waves: lane tx < TY+2 completes the x-halo cell of tile row tx (other lanes repeat their own cell: no branches around loads)
  const bool hwave = ty == 0 || ty == TY + 1;
  const int sside = ty == 0 ? 0 : 1, hxs = sside ? 65 : 0, si0 = bx * 64 + (sside ? 65 : 0), sj0 = by * TY + tx - EXT;
  const bool sok = hwave && tx < TY + 2 && sj0 <= n2 + 1 + EXT;
  const int si = !sok ? i : si0 == 0 ? n1 : si0 == n1 + 1 ? 1 : si0, sjr = !sok ? jq : urow(sj0), sjx = !sok ? j : sj0;
  const int sxr = si >= n1 ? 1 : si + 1;
  const OFF so = foff(si, sjx, NCV), sop = foff(si, sjx, NCP), soy = foff(si, sjx + 1, NCP), sox = foff(sxr, sjx, NCP);
  const int srow = sok ? tx : 0;
  auto kz = [&](int kk) { return !A.zper ? kk : kk == 0 ? n3 : kk == n3 + 1 ? 1 : kk; };      // plane that holds the values of plane kk
  const real f0 = (A.fmask & 1) ? ldc(A.force, 0) : 0., f1 = (A.fmask & 2) ? ldc(A.force, 1) : 0., f2 = (A.fmask & 4) ? ldc(A.force, 2) : 0.;
  // what is in flight for one column between two iterations: the prediction of a plane and pp of the cell above it (k+1); the side job's column also
  // loads its pp(i+1) and pp(j+1), the own cells find theirs in sP (the top halo row, whose row above is another block's, loads its pp(j+1))
  struct Raw { real q[3], pz; };
  struct RawS { real q[3], pz, px, py; };
  auto rawload = [&](int kk, Raw &r) {      // kk: a plane index in 0..n3+1 (mapped by kz)
    const OFF a = cl + (OFF)kk * sk;
#pragma unroll
    for (int q = 0; q < 3; ++q) r.q[q] = ldb(A.u[q], a);
    r.pz = ldb(A.pp, clp + (OFF)min(kk + 1, n3 + 1) * sk);
  };
  auto rawloads = [&](int kk, RawS &r) {
    const OFF a = so + (OFF)kk * sk;
#pragma unroll
    for (int q = 0; q < 3; ++q) r.q[q] = ldb(A.u[q], a);
    r.pz = ldb(A.pp, sop + (OFF)min(kk + 1, n3 + 1) * sk); r.px = ldb(A.pp, sox + (OFF)kk * sk); r.py = ldb(A.pp, soy + (OFF)kk * sk);
  };
  // interior plane kq: (u* + f) - dtrk grad(pp), k_correc_cell's operations in their order
  auto fix = [&](const real *q, real P0, real px, real py, real pz, int kq, real *o) {
    o[0] = ((A.fmask & 1) ? q[0] + f0 : q[0]) - A.cfi * (px - P0);
    o[1] = ((A.fmask & 2) ? q[1] + f1 : q[1]) - A.cfj * (py - P0);
    o[2] = ((A.fmask & 4) ? q[2] + f2 : q[2]) - A.cdt * ldc(A.dzci, kq) * (pz - P0);
  };
  // ghost plane next to a wall (sd = 0: plane 0, 1: plane n3+1): u, v = 2 bc - (the plane beside it, bes[]) as bounduvw sets them, w(0) by the formula
  // without forcing (correc.f90 covers k = 0..n3 for w), w(n3+1) untouched (bounduvw with is_correc leaves the normal component's z faces alone)
  auto wallfix = [&](const real *q, real P0, real pz, int sd, size_t qbc, const real *bes, real *o) {
    o[0] = 2. * A.bcz[0][sd][qbc] - bes[0]; o[1] = 2. * A.bcz[1][sd][qbc] - bes[1];
    o[2] = sd == 0 ? q[2] - A.cdt * ldc(A.dzci, 0) * (pz - P0) : q[2];
  };
  const size_t q2 = (size_t)i + (size_t)(n1 + 2) * jq, q2s = (size_t)si + (size_t)(n1 + 2) * sjr;
  Raw rn; RawS rh = {}; real p0n, p0h = 0., pyt = 0.;      // in flight at the top of iteration k: plane k+1 of the own / the side job's column, pp of its cell, p of the own cell; pyt: pp(j+1) of the top halo row
  { // ---- planes kbeg-1 and kbeg complete, plane kbeg+1 in flight (pp's neighbours by direct loads here: sP serves the loop)
    real c1[3], c0v[3], h1[3] = {0., 0., 0.}, h0[3] = {0., 0., 0.};
    const bool low = !A.zper && kbeg == 1;      // plane kbeg-1 is the ghost plane below the lower wall
    const OFF clx = foff(i >= n1 ? 1 : i + 1, j, NCP);
    { const int kq = kz(kbeg); Raw r; rawload(kq, r); const real P0 = ldb(A.pp, clp + (OFF)kq * sk);
      fix(r.q, P0, ldb(A.pp, clx + (OFF)kq * sk), ldb(A.pp, cly + (OFF)kq * sk), r.pz, kq, c1); p0n = r.pz;
      const OFF a = cst + (OFF)kbeg * sk; stb(A.p, a, ldb(A.p, a) + P0);      // p += pp (updatep.f90:30-47, explicit diffusion); lanes without output: their ghost cell
      if (hwave) { RawS e; rawloads(kq, e); const real E0 = ldb(A.pp, sop + (OFF)kq * sk); fix(e.q, E0, e.px, e.py, e.pz, kq, h1); p0h = e.pz; } }
    { const int kq = kz(kbeg - 1); Raw r; rawload(kq, r); const real P0 = ldb(A.pp, clp + (OFF)kq * sk);
      if (low) wallfix(r.q, P0, r.pz, 0, q2, c1, c0v); else fix(r.q, P0, ldb(A.pp, clx + (OFF)kq * sk), ldb(A.pp, cly + (OFF)kq * sk), r.pz, kq, c0v);
      if (hwave) { RawS e; rawloads(kq, e); const real E0 = ldb(A.pp, sop + (OFF)kq * sk);
                   if (low) wallfix(e.q, E0, e.pz, 0, q2s, h1, h0); else fix(e.q, E0, e.px, e.py, e.pz, kq, h0); } }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      ring[(kbeg - 1) % 3][q][ty][tx + 1] = c0v[q]; ring[kbeg % 3][q][ty][tx + 1] = c1[q];
      if (sok) { ring[(kbeg - 1) % 3][q][srow][hxs] = h0[q]; ring[kbeg % 3][q][srow][hxs] = h1[q]; }
      stb(A.un[q], cst + (OFF)kbeg * sk, c1[q]);
    }
    sP[(kbeg + 1) & 1][ty][tx] = p0n;      // pp of plane kbeg+1
    if (sok && sside) sP[(kbeg + 1) & 1][srow][64] = p0h;
    rawload(kz(kbeg + 1), rn);
    if (hwave) { rawloads(kz(kbeg + 1), rh); pyt = ldb(A.pp, cly + (OFF)kz(kbeg + 1) * sk); }
    __syncthreads();
  }
  int km = (kbeg - 1) % 3, kc = kbeg % 3, kp = (kbeg + 1) % 3;
  real keep[3] = {0., 0., 0.};
  // one plane. HALO: a y-halo wave (side job, no outputs); TOP: plane k+1 is the ghost plane above the upper wall (k = n3, walls)
  auto plane = [&](const int k, auto halo_c, auto top_c) {
    constexpr bool HALO = decltype(halo_c)::value, TOP = decltype(top_c)::value;
    const OFF idx = cst + (OFF)k * sk;
    { // plane k+1, loaded during the last iteration, is completed, stored if it belongs to this chunk, and plane k+2 goes into flight
      const int par = (k + 1) & 1, k2 = kz(min(k + 2, n3 + 1));
      real cc[3];
      if (TOP) { const real bes[2] = {ring[kc][0][ty][tx + 1], ring[kc][1][ty][tx + 1]}; wallfix(rn.q, p0n, rn.pz, 1, q2, bes, cc); }
      else {
        real px = lane_next(p0n);
        if (tx == 63) px = sP[par][ty][64];
        const real py = (HALO && ty == TY + 1) ? pyt : sP[par][ty + (ty == TY + 1 ? 0 : 1)][tx];
        fix(rn.q, p0n, px, py, rn.pz, kz(k + 1), cc);
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) ring[kp][q][ty][tx + 1] = cc[q];
      sP[par ^ 1][ty][tx] = rn.pz;      // pp of plane k+2
      if (!HALO) {
        // (plane k+1 of the NEXT chunk, or the ghost plane n3+1, goes to the row's x ghost cell like the results of lanes without output)
        const OFF dst = (outok && k + 1 <= kend ? cst : cdump) + (OFF)(k + 1) * sk;
#pragma unroll
        for (int q = 0; q < 3; ++q) stb(A.un[q], dst, cc[q]);
      }
      p0n = rn.pz;
      rawload(k2, rn);
      // (the data registers of the last plane's three filtered-velocity stores stay allocated up to here: reused earlier, the compiler has to wait
      //  for those stores -- the youngest operations in flight, i.e. for everything -- before the first instruction that overwrites them)
      if (!HALO) asm volatile("" :: "v"(keep[0]), "v"(keep[1]), "v"(keep[2]));
      if (HALO) {
        real hh[3];
        if (TOP) { const real hbes[2] = {ring[kc][0][srow][hxs], ring[kc][1][srow][hxs]}; wallfix(rh.q, p0h, rh.pz, 1, q2s, hbes, hh); }
        else fix(rh.q, p0h, sside ? rh.px : sP[par][srow][0], rh.py, rh.pz, kz(k + 1), hh);
        if (sok) {
#pragma unroll
          for (int q = 0; q < 3; ++q) ring[kp][q][srow][hxs] = hh[q];
          if (sside) sP[par ^ 1][srow][64] = rh.pz;
        }
        p0h = rh.pz;
        rawloads(k2, rh);
        pyt = ldb(A.pp, cly + (OFF)k2 * sk);
      }
    }
    __syncthreads();
    // p += pp of plane k+1 (updatep.f90:30-47, explicit diffusion): loaded here, stored behind the second barrier -- load, wait and store inside one
    // iteration, nothing of it carried around the loop; pp(k+1) of the cell is still in sP
    const OFF dstp = (outok && k + 1 <= kend ? cst : cdump) + (OFF)(k + 1) * sk;
    real pl = 0.;
    if (!HALO) pl = ldb(A.p, dstp);
    const bool lo = A.zlo && k == 1, hi = A.zhi && k == n3;
    real r[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      auto zcomb = [&](int x) {
        const real qm = ring[km][q][ty][x], qc = ring[kc][q][ty][x], qp = ring[kp][q][ty][x];
        const real vm = (lo && q < 2) ? 2. * qc - qp : qm;      // u,v extrapolated through the walls, w (on the faces) not
        const real vp = (hi && q < 2) ? 2. * qc - qm : qp;
        return vm + 2. * qc + vp;
      };
      const real G = zcomb(tx + 1);
      real pv = lane_prev(G), nx = lane_next(G);
      if (edge) { const real Gh = zcomb(hx); if (tx == 0) pv = Gh; else nx = Gh; }
      r[q] = pv + 2. * G + nx;
      shs[q][ty][tx] = r[q];
    }
    if (!HALO) {
#define RU(dk, dj, di) ring[dk][0][ty + (dj)][tx + 1 + (di)]
#define RV(dk, dj, di) ring[dk][1][ty + (dj)][tx + 1 + (di)]
#define RW(dk, dj, di) ring[dk][2][ty + (dj)][tx + 1 + (di)]
      // the thirty ring values are read group by group (the scheduling barriers keep the compiler from hoisting all LDS reads to the top, which costs
      // the fourteen registers this pass does not have at sixteen waves per block); expressions and their order as in k_strain_tile
      const real dxi = A.dxi, dyi = A.dyi, zc = ldc(A.dzci, k), zm = ldc(A.dzci, k - 1);
      const real u_ccc = RU(kc, 0, 0), u_mcc = RU(kc, 0, -1), v_ccc = RV(kc, 0, 0), v_cmc = RV(kc, -1, 0), w_ccc = RW(kc, 0, 0), w_ccm = RW(km, 0, 0);
      const real s11 = (u_ccc - u_mcc) * dxi, s22 = (v_ccc - v_cmc) * dyi, s33 = (w_ccc - w_ccm) * ldc(A.dzfi, k);
      real s12, s13, s23;
      { const real u_mmc = RU(kc, -1, -1), u_cmc = RU(kc, -1, 0), u_mpc = RU(kc, 1, -1), u_cpc = RU(kc, 1, 0);
        const real v_mmc = RV(kc, -1, -1), v_pmc = RV(kc, -1, 1), v_mcc = RV(kc, 0, -1), v_pcc = RV(kc, 0, 1);
        s12 = .125 * ((u_cpc - u_ccc) * dyi + (v_pcc - v_ccc) * dxi + (u_ccc - u_cmc) * dyi + (v_pmc - v_cmc) * dxi +
                      (u_mpc - u_mcc) * dyi + (v_ccc - v_mcc) * dxi + (u_mcc - u_mmc) * dyi + (v_cmc - v_mmc) * dxi); }
      __builtin_amdgcn_sched_barrier(0);
      { const real u_mcm = RU(km, 0, -1), u_ccm = RU(km, 0, 0), u_mcp = RU(kp, 0, -1), u_ccp = RU(kp, 0, 0);
        const real w_mcm = RW(km, 0, -1), w_pcm = RW(km, 0, 1), w_mcc = RW(kc, 0, -1), w_pcc = RW(kc, 0, 1);
        s13 = .125 * ((u_ccp - u_ccc) * zc + (w_pcc - w_ccc) * dxi + (u_ccc - u_ccm) * zm + (w_pcm - w_ccm) * dxi +
                      (u_mcp - u_mcc) * zc + (w_ccc - w_mcc) * dxi + (u_mcc - u_mcm) * zm + (w_ccm - w_mcm) * dxi); }
      __builtin_amdgcn_sched_barrier(0);
      { const real v_cmm = RV(km, -1, 0), v_ccm = RV(km, 0, 0), v_cmp = RV(kp, -1, 0), v_ccp = RV(kp, 0, 0);
        const real w_cmm = RW(km, -1, 0), w_cpm = RW(km, 1, 0), w_cmc = RW(kc, -1, 0), w_cpc = RW(kc, 1, 0);
        s23 = .125 * ((v_ccp - v_ccc) * zc + (w_cpc - w_ccc) * dyi + (v_ccc - v_ccm) * zm + (w_cpm - w_ccm) * dyi +
                      (v_cmp - v_cmc) * zc + (w_ccc - w_cmc) * dyi + (v_cmc - v_cmm) * zm + (w_ccm - w_cmm) * dyi); }
#undef RU
#undef RV
#undef RW
      const real s0v = sqrt(2. * (s11 * s11 + s22 * s22 + s33 * s33 + 2. * (s12 * s12 + s13 * s13 + s23 * s23)));
      stb(A.s0, idx, s0v);                                              // stands for visct = s0 (sgs.f90:184) until the final kernel
      const OFF i2 = 2 * idx;      // |S|Sij (sgs.f90:198-210), two components per 16-byte store
      typedef real v2 __attribute__((ext_vector_type(2)));
      __builtin_nontemporal_store(v2{s0v * s11, s0v * s22}, (v2 *)((char *)A.ss2[0] + i2));
      if (FIVE) __builtin_nontemporal_store(s0v * s12, (real *)((char *)A.ss2[1] + idx));
      else __builtin_nontemporal_store(v2{s0v * s33, s0v * s12}, (v2 *)((char *)A.ss2[1] + i2));
      __builtin_nontemporal_store(v2{s0v * s13, s0v * s23}, (v2 *)((char *)A.ss2[2] + i2));
      // (the cell-centred velocity is not stored: the last pass forms it from u, v, w itself -- the only form this pass serves, dsmag_fast)
      // EXT: v_c of the two ghost rows, which the last pass reads from A.vcg (row 0: its lower neighbour v(-1) is in this tile's ring, nowhere else);
      // every other row stores to its dump cell -- no branch around the store
      if (EXT) stb(A.vcg, cvc + (OFF)k * sk, 0.5 * (v_ccc + v_cmc));
    }
    __syncthreads();
    if (!HALO) {
#pragma unroll
      for (int q = 0; q < 3; ++q) { keep[q] = (shs[q][ty - 1][tx] + 2. * r[q] + shs[q][ty + 1][tx]) / 64.; stb(A.uf[q], idx, keep[q]); }
      stb(A.p, dstp, pl + sP[(k + 1) & 1][ty][tx]);
    }
    const int t = km; km = kc; kc = kp; kp = t;
  };
  const std::true_type T_; const std::false_type F_;
  const bool topw = !A.zper && kend == n3;      // the chunk's last plane sits under the upper wall
  const int klast = topw ? kend - 1 : kend;
  // (a wave's row is uniform: scalar branches, each loop straight-line code)
  // The first plane is peeled off: the loop is then entered with the same operations in flight as its back edge carries (the loads of a plane with
  // that plane's stores behind them), and the compiler's counted waits hold; entered from the prologue, whose last operation is a load, the merge of
  // the two states at the loop header makes every wait a wait for everything.
  if (__builtin_amdgcn_readfirstlane((int)hwave)) {
    if (kbeg <= klast) plane(kbeg, T_, F_);
    for (int k = kbeg + 1; k <= klast; ++k) plane(k, T_, F_);
    if (topw) plane(kend, T_, T_);
  } else {
    if (kbeg <= klast) plane(kbeg, F_, F_);
    for (int k = kbeg + 1; k <= klast; ++k) plane(k, F_, F_);
    if (topw) plane(kend, F_, T_);
  }
}
// Static Smagorinsky, row-marching form (default): one wave per row of 62 cells marching in k with everything in registers -- x neighbours by
// DPP lane moves, the rows j-1 and j+1 loaded again by this wave (they are their own waves' rows: cache hits), z neighbours rolled from plane
// to plane. No LDS and no barriers: the tile form above is bound by its barrier pair per plane with two square roots and an exponential per
// cell in between (0.26 of the HBM peak); here waves never wait for each other and the VGPR count alone sets the occupancy.
// (sgs.f90:98-152, 598-680)
constexpr int SROWS = 4;      // rows (waves) per block
// EX = 1: the block holds a row next to a wall-model y face (block-uniform: the other blocks of a duct run the loads of the channel form).
// Every global access of the plane loop is straight-line code ("In-order counters"): the extrapolated ghost row is c1 Q(o1) - c2 Q(o2)
// with per-thread offsets and weights instead of a branch around two loads, the shear of the nearer y wall is loaded for every plane whether the
// nearest wall turns out to be that one or a z wall -- the branches of the first version made each of the plane's loads a round trip of its own
// (0.50 ms per call for the 512 x 256 x 256 duct against 0.37 ms now).
template <typename OFF, int YW, int EX>
__device__ __forceinline__ void smag_rows_body(const Geom &g, const StrainTileArgs &A, const int bx, const int by, const int bz) {
  const int tx = threadIdx.x;
  const int i = bx * 62 + tx, j = by * SROWS + threadIdx.y + 1;
  if (j > g.n2) return;
  const int kbeg = bz * A.kchunk + 1, kend = min(kbeg + A.kchunk - 1, g.n3);
  const bool ldok = i <= g.n1 + 1, outok = tx >= 1 && tx <= 62 && i <= g.n1;
  const OFF sj = (OFF)g.s1 * RSZ, sk = (OFF)g.s12 * RSZ;
  const int iw = !A.perx ? i : i == 0 ? g.n1 : i == g.n1 + 1 ? 1 : i;      // periodic x: wrapped columns instead of the ghost columns
  const OFF c0 = ldok ? (OFF)g.ix(iw, j, 0) * RSZ : (OFF)g.ix(1, j, 0) * RSZ;
  // ghost rows at wall-model y faces: u and w are replaced by 2 Q(1) - Q(2) along y; v, normal to the face, is not (extrapolate(...,lwm), sgs.f90:683-748)
  const bool exlo = EX && A.wmylo && j == 1, exhi = EX && A.wmyhi && j == g.n2;
  // (lanes beyond the row read cell 0 of the field and planes beyond n3+1 are clamped: every load is unconditional, nothing branches around it)
  const OFF a1 = exlo ? c0 : c0 - sj, a2 = exlo ? c0 + sj : c0 - sj, b1 = exhi ? c0 : c0 + sj, b2 = exhi ? c0 - sj : c0 + sj;      // rows j-1 (a) and j+1 (b)
  const real ac1 = exlo ? 2. : 1., ac2 = exlo ? 1. : 0., bc1 = exhi ? 2. : 1., bc2 = exhi ? 1. : 0.;
  auto ldu = [&](int q, int dj, int k) -> real {      // q = 0 (u) or 2 (w), dj = -1, 0, +1
    const OFF o = (OFF)k * sk;
    if (EX && dj < 0) return ac1 * ldb(A.u[q], a1 + o) - ac2 * ldb(A.u[q], a2 + o);
    if (EX && dj > 0) return bc1 * ldb(A.u[q], b1 + o) - bc2 * ldb(A.u[q], b2 + o);
    return ldb(A.u[q], dj < 0 ? c0 + o - sj : dj > 0 ? c0 + o + sj : c0 + o);
  };
  auto ldv = [&](int dj, int k) -> real { return ldb(A.u[1], c0 + (OFF)k * sk - (dj < 0 ? sj : 0)); };
  // planes k-1, k, k+1 of u(j), v(j-1), v(j); plane k of u(j-1), u(j+1); planes k-1, k of w(j-1), w(j), w(j+1)
  real u0m = ldu(0, 0, kbeg - 1), u0c = ldu(0, 0, kbeg), u0p = ldu(0, 0, kbeg + 1);
  real vAm = ldv(-1, kbeg - 1), vAc = ldv(-1, kbeg), vAp = ldv(-1, kbeg + 1);
  real vCm = ldv(0, kbeg - 1), vCc = ldv(0, kbeg), vCp = ldv(0, kbeg + 1);
  real uA = ldu(0, -1, kbeg), uB = ldu(0, 1, kbeg);
  real wAm = ldu(2, -1, kbeg - 1), wCm = ldu(2, 0, kbeg - 1), wBm = ldu(2, 1, kbeg - 1);
  real wAc = ldu(2, -1, kbeg), wCc = ldu(2, 0, kbeg), wBc = ldu(2, 1, kbeg);
  // van Driest: wall units from the shear at the nearer z wall of this column (sgs.f90:117-143), read from the fields themselves
  // (their ghost cells, not the extrapolated ones)
  real tw_lo = 0., tw_hi = 0.;
  if (outok) {
    const real *u = A.u[0], *v = A.u[1];
    const int im1 = (A.perx && i == 1) ? g.n1 : i - 1;
    if (A.zlo) {
      const real t1 = u[g.ix(i, j, 1)] - u[g.ix(i, j, 0)] + u[g.ix(im1, j, 1)] - u[g.ix(im1, j, 0)];
      const real t2 = v[g.ix(i, j, 1)] - v[g.ix(i, j, 0)] + v[g.ix(i, j - 1, 1)] - v[g.ix(i, j - 1, 0)];
      tw_lo = sqrt(0.5 * A.visc * (sqrt(t1 * t1 + t2 * t2) * A.dzci[0]));
    }
    if (A.zhi) {
      const int n3 = g.n3;
      const real t1 = u[g.ix(i, j, n3)] - u[g.ix(i, j, n3 + 1)] + u[g.ix(im1, j, n3)] - u[g.ix(im1, j, n3 + 1)];
      const real t2 = v[g.ix(i, j, n3)] - v[g.ix(i, j, n3 + 1)] + v[g.ix(i, j - 1, n3)] - v[g.ix(i, j - 1, n3 + 1)];
      tw_hi = sqrt(0.5 * A.visc * (sqrt(t1 * t1 + t2 * t2) * A.dzci[n3]));
    }
  }
  const real dxi = A.dxi, dyi = A.dyi;
  // van Driest with y walls: the nearer y wall of this row (the first one wins a tie) is known before the loop; its shear plane is read for every k
  const int jg = j + g.jlo;
  real dminy = YW && A.wylo ? A.dl2 * (jg - 0.5) : CALES_BIG; int locy = 2;
  { const real d = YW && A.wyhi ? A.dl2 * (g.ng2 - jg + 0.5) : CALES_BIG; if (d < dminy) { dminy = d; locy = 3; } }
  const real *twp = (YW && A.twy) ? A.twy + (size_t)(locy == 3 ? g.n3 + 2 : 0) * g.s1 + (ldok ? i : 1) : A.del;
  const int tws = (YW && A.twy) ? g.s1 : 0;
  real twyc = YW ? twp[(size_t)kbeg * tws] : 0.;
  for (int k = kbeg; k <= kend; ++k) {
    // next iteration's planes, in flight during this one's arithmetic
    const int k2 = min(k + 2, g.n3 + 1), k1 = k + 1;
    const real twyn = YW ? twp[(size_t)k1 * tws] : 0.;
    const real u0n = ldu(0, 0, k2), vAn = ldv(-1, k2), vCn = ldv(0, k2);
    const real uAn = ldu(0, -1, k1), uBn = ldu(0, 1, k1);
    const real wAn = ldu(2, -1, k1), wCn = ldu(2, 0, k1), wBn = ldu(2, 1, k1);
    // wall-model z faces: ghost planes of u, v by extrapolation with the grid factor
    real u_ccm = u0m, v_cmm = vAm, v_ccm = vCm, u_ccp = u0p, v_cmp = vAp, v_ccp = vCp;
    if (A.wmlo && k == 1) { u_ccm = (1. + A.flo) * u0c - A.flo * u0p; v_cmm = (1. + A.flo) * vAc - A.flo * vAp; v_ccm = (1. + A.flo) * vCc - A.flo * vCp; }
    if (A.wmhi && k == g.n3) { u_ccp = (1. + A.fhi) * u0c - A.fhi * u0m; v_cmp = (1. + A.fhi) * vAc - A.fhi * vAm; v_ccp = (1. + A.fhi) * vCc - A.fhi * vCm; }
    const real u_ccc = u0c, u_cmc = uA, u_cpc = uB, v_cmc = vAc, v_ccc = vCc;
    const real w_cmm = wAm, w_ccm = wCm, w_cpm = wBm, w_cmc = wAc, w_ccc = wCc, w_cpc = wBc;
    const real u_mcm = lane_prev(u_ccm), u_mcc = lane_prev(u_ccc), u_mcp = lane_prev(u_ccp), u_mmc = lane_prev(u_cmc), u_mpc = lane_prev(u_cpc);
    const real v_mmc = lane_prev(v_cmc), v_pmc = lane_next(v_cmc), v_mcc = lane_prev(v_ccc), v_pcc = lane_next(v_ccc);
    const real w_mcm = lane_prev(w_ccm), w_pcm = lane_next(w_ccm), w_mcc = lane_prev(w_ccc), w_pcc = lane_next(w_ccc);
    const real zc = ldc(A.dzci, k), zm = ldc(A.dzci, k - 1);
    const real s11 = (u_ccc - u_mcc) * dxi, s22 = (v_ccc - v_cmc) * dyi, s33 = (w_ccc - w_ccm) * ldc(A.dzfi, k);
    const real s12 = .125 * ((u_cpc - u_ccc) * dyi + (v_pcc - v_ccc) * dxi + (u_ccc - u_cmc) * dyi + (v_pmc - v_cmc) * dxi +
                               (u_mpc - u_mcc) * dyi + (v_ccc - v_mcc) * dxi + (u_mcc - u_mmc) * dyi + (v_cmc - v_mmc) * dxi);
    const real s13 = .125 * ((u_ccp - u_ccc) * zc + (w_pcc - w_ccc) * dxi + (u_ccc - u_ccm) * zm + (w_pcm - w_ccm) * dxi +
                               (u_mcp - u_mcc) * zc + (w_ccc - w_mcc) * dxi + (u_mcc - u_mcm) * zm + (w_ccm - w_mcm) * dxi);
    const real s23 = .125 * ((v_ccp - v_ccc) * zc + (w_cpc - w_ccc) * dyi + (v_ccc - v_ccm) * zm + (w_cpm - w_ccm) * dyi +
                               (v_cmp - v_cmc) * zc + (w_ccc - w_cmc) * dyi + (v_cmc - v_cmm) * zm + (w_ccm - w_cmm) * dyi);
    const real s0v = sqrt(2. * (s11 * s11 + s22 * s22 + s33 * s33 + 2. * (s12 * s12 + s13 * s13 + s23 * s23)));
    if (outok) {
      real fd = 1.;
      if (A.zlo || A.zhi || (YW && (A.wylo || A.wyhi))) {     // nearest wall in the order y-, y+, z-, z+: the first one wins a tie (minloc, sgs.f90:116)
        real dmin = dminy; int loc = locy;
        { const real d = A.zlo ? ldc(A.zc, k) : CALES_BIG; if (d < dmin) { dmin = d; loc = 4; } }
        { const real d = A.zhi ? A.l3 - ldc(A.zc, k) : CALES_BIG; if (d < dmin) { dmin = d; loc = 5; } }
        const real tw = loc < 4 ? twyc : loc == 4 ? tw_lo : tw_hi;
        const real dw_plus = dmin * tw * (1. / A.visc);
        fd = 1. - exp(-dw_plus / 25.);
      }
      const real t = 0.11 * ldc(A.del, k) * fd;      // c_smag, src/param.f90:33
      stb(A.visct, c0 + (OFF)k * sk, (t * t) * s0v);
    }
    u0m = u0c; u0c = u0p; u0p = u0n; vAm = vAc; vAc = vAp; vAp = vAn; vCm = vCc; vCc = vCp; vCp = vCn;
    uA = uAn; uB = uBn; wAm = wAc; wCm = wCc; wBm = wBc; wAc = wAn; wCc = wCn; wBc = wBn;
    twyc = twyn;
  }
}
template <typename OFF, int YW>
// (four waves per SIMD -- 128 VGPRs -- for channels; the duct logic needs a few registers more and would spill under that cap)
__global__ __launch_bounds__(64 * SROWS, (YW ? 3 : 4)) void k_smag_rows(Geom g, StrainTileArgs A) {
  // band map (common.hpp): the rows two waves both load (j-1, j+1, the shared columns of neighbouring x tiles) meet in one L2 instead of
  // being fetched from memory by two (measured 1.8 x the compulsory reads with the plain 3-D grid, 1.27 x with the bands)
  int bx, by, bz;
  if (!band_block(A.bm, bx, by, bz)) return;
  if (YW && ((A.wmylo && by == 0) || (A.wmyhi && (by + 1) * SROWS >= g.n2))) smag_rows_body<OFF, YW, 1>(g, A, bx, by, bz);
  else smag_rows_body<OFF, YW, 0>(g, A, bx, by, bz);
}
// p1d[which*n3 + k-1] = sum over the blocks' partials, fixed order (ave1d_channel, sgs.f90:462-472)
__global__ __launch_bounds__(256) void k_plane_fold(int n3, int nblk, const real *__restrict__ part, real *__restrict__ p1d) {
  __shared__ real sh[4];
  const real *p = part + (size_t)blockIdx.x * nblk;
  real acc = 0.;
  for (int q = threadIdx.x; q < nblk; q += 256) acc += p[q];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) p1d[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
  (void)n3;
}

// v_c = (v(j) + v(j-1))/2 of the rows j = 1 and j = n2 (all i, k, ghost columns and planes included): the two rows whose copies the ghost-cell update /
// the slab exchange puts into the ghost rows 0 and n2+1 of `vc` -- k_lmf_tile<.., UCF = 1> reads row 0 from there
__global__ __launch_bounds__(256) void k_vc_edge_rows(Geom g, const real *__restrict__ v, real *__restrict__ vc) {
  const int i = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y * 4 + threadIdx.y;
  if (i > g.n1 + 1 || k > g.n3 + 1) return;
  vc[g.ix(i, 1, k)] = 0.5 * (v[g.ix(i, 1, k)] + v[g.ix(i, 0, k)]);
  vc[g.ix(i, g.n2, k)] = 0.5 * (v[g.ix(i, g.n2, k)] + v[g.ix(i, g.n2 - 1, k)]);
}
// z faces of the normal velocity after a projection folded into k_corr_strain_tile (which writes the planes 1..n3): plane 0 is corrected like
// every other (correc.f90:60-66: k = 0..n3, ghost rows and columns included), plane n3+1 keeps the value the last bounduvw gave the prediction
__global__ __launch_bounds__(256) void k_wface_fold(Geom g, const real *__restrict__ ws, real *__restrict__ wd, const real *__restrict__ pp, real cz0) {
  const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
  if (i > g.n1 + 1 || j > g.n2 + 1) return;
  const size_t a = g.ix(i, j, 0), b = g.ix(i, j, g.n3 + 1);
  wd[a] = ws[a] - cz0 * (pp[a + g.s12] - pp[a]);
  wd[b] = ws[b];
}
// Several slabs, projection folded into the strain-rate pass: the corrected velocity and p + pp of the two GHOST rows (the neighbours' rows n2 and 1) are
// formed HERE, from the prediction's ghost rows and pp's -- the operands the neighbour's own pass has for those rows, the operations of `fix` in
// k_corr_strain_tile (correc.f90:44-67, updatep.f90:30-47) in their order -- instead of travelling: four field planes per substep less in the slab
// exchange (63 -> 51 planes per step). pp of "row n2+2" for v in the upper ghost row: the companion field (api.hip). Interior
// cells i = 1..n1, k = 1..n3 of the two rows; their x and z ghost cells follow from the ghost-cell kernel, whose loops cover the ghost rows, and
// plane 0 of w from k_wface_fold.
__global__ __launch_bounds__(256) void k_fold_ghost_rows(Geom g, const real *__restrict__ us, const real *__restrict__ vs, const real *__restrict__ ws,
                                                         real *__restrict__ ud, real *__restrict__ vd, real *__restrict__ wd, const real *__restrict__ pp,
                                                         const real *__restrict__ ppc, real *__restrict__ p, const real *__restrict__ force, int fmask,
                                                         real cfi, real cfj, real cdt, const real *__restrict__ dzci, int perx) {
  const int i = blockIdx.x * 64 + threadIdx.x + 1, k = blockIdx.y * 4 + threadIdx.y + 1, side = blockIdx.z;
  if (i > g.n1 || k > g.n3) return;
  const int j = side ? g.n2 + 1 : 0, ip = (perx && i == g.n1) ? 1 : i + 1;
  const size_t a = g.ix(i, j, k);
  const real P0 = pp[a], px = pp[g.ix(ip, j, k)], py = side ? ppc[a] : pp[a + g.s1], pz = pp[a + g.s12];
  const real f0 = (fmask & 1) ? force[0] : 0., f1 = (fmask & 2) ? force[1] : 0., f2 = (fmask & 4) ? force[2] : 0.;
  ud[a] = ((fmask & 1) ? us[a] + f0 : us[a]) - cfi * (px - P0);
  vd[a] = ((fmask & 2) ? vs[a] + f1 : vs[a]) - cfj * (py - P0);
  wd[a] = ((fmask & 4) ? ws[a] + f2 : ws[a]) - cdt * dzci[k] * (pz - P0);
  p[a] = p[a] + P0;
}
// ---- the path of cmpt_sgs (SgsPath, common.hpp). The kernel records first: one function per kernel family, every instantiation named ONCE, picked by the properties that
// select it; sgs_setup is their only caller. The launch check reports a record's name as spelled here and tests match it: the numbers stay numbers. Not built: an empty record
using StrainKernelRec = KernelRec<void(Geom, StrainTileArgs)>; using LmfKernelRec = KernelRec<void(Geom, LmfArgs)>;
// K_AC. Pair fields and the plane filter imply no y logic, pair fields 32-bit offsets too: one instantiation, two
static StrainKernelRec strain_kernel(bool pair, bool f2d, bool yw, bool small) {
  static_assert(STRAIN_PAIR == 1 && STRAIN_F2D == 2, "SSF as spelled below");
  static const StrainKernelRec plain[2][2] = {{KERNEL_REC(k_strain_tile<size_t, TYS, 0>), KERNEL_REC(k_strain_tile<unsigned, TYS, 0>)}, {KERNEL_REC(k_strain_tile<size_t, TYS, 1>), KERNEL_REC(k_strain_tile<unsigned, TYS, 1>)}};      // [yw][small]
  static const StrainKernelRec plane[2] = {KERNEL_REC(k_strain_tile<size_t, TYS, 0, 2>), KERNEL_REC(k_strain_tile<unsigned, TYS, 0, 2>)}, pairs = KERNEL_REC(k_strain_tile<unsigned, TYS, 0, 1>);      // [small]
  return pair ? pairs : f2d ? plane[small] : plain[yw][small];
}
// K_AC with the projection folded in (pair fields). rows2: from two ghost rows of the prediction (several slabs); five components: one rank
static StrainKernelRec corr_strain_kernel(bool rows2, bool five) {
  static const StrainKernelRec t[2][2] = {{KERNEL_REC(k_corr_strain_tile<unsigned, TYC>), KERNEL_REC(k_corr_strain_tile<unsigned, TYC, 2>)}, {KERNEL_REC(k_corr_strain_tile<unsigned, TYC, 1>), {}}};      // [rows2][five]
  return t[rows2][five];
}
// The last pass. pair: 0 | LMF_PAIR | LMF_PAIR5 (x and y periodic, ucf, 32-bit offsets: one instantiation each, and one more each for the packed remainder tile). local: built for
// ucf with 32-bit offsets (with 64-bit ones it spills: profiles/dsmag_local_kernel_resources.md), six components, the 3-D filter; every other: empty, sgs_setup takes the sequence
static LmfKernelRec lmf_kernel(bool f2d, int pair, bool local, bool packed, bool yw, bool ucf, bool small) {
  static_assert(LMF_PAIR == 1 && LMF_PAIR5 == 2 && LMF_LOCAL == 4 && (LMF_LOCAL | LMF_PAIR) == 5 && (LMF_PACK | LMF_PAIR) == 9 && (LMF_PACK | LMF_PAIR5) == 10, "SSF as spelled below");
  static const LmfKernelRec six[2][2][2] = {{{KERNEL_REC(k_lmf_tile<size_t, 0, 0>), KERNEL_REC(k_lmf_tile<unsigned, 0, 0>)}, {KERNEL_REC(k_lmf_tile<size_t, 0, 1>), KERNEL_REC(k_lmf_tile<unsigned, 0, 1>)}},
                                            {{KERNEL_REC(k_lmf_tile<size_t, 1, 0>), KERNEL_REC(k_lmf_tile<unsigned, 1, 0>)}, {KERNEL_REC(k_lmf_tile<size_t, 1, 1>), KERNEL_REC(k_lmf_tile<unsigned, 1, 1>)}}};      // [yw][ucf][small]
  static const LmfKernelRec plane[2] = {KERNEL_REC(k_lmf_plane_tile<size_t>), KERNEL_REC(k_lmf_plane_tile<unsigned>)};      // [small]
  static const LmfKernelRec pairs[3] = {{}, KERNEL_REC(k_lmf_tile<unsigned, 0, 1, 1>), KERNEL_REC(k_lmf_tile<unsigned, 0, 1, 2>)};      // [pair]
  static const LmfKernelRec packs[3] = {{}, KERNEL_REC(k_lmf_tile<unsigned, 0, 1, 9>), KERNEL_REC(k_lmf_tile<unsigned, 0, 1, 10>)};      // [pair]
  static const LmfKernelRec locals[2] = {KERNEL_REC(k_lmf_tile<unsigned, 0, 1, 4>), KERNEL_REC(k_lmf_tile<unsigned, 1, 1, 4>)}, local_pairs = KERNEL_REC(k_lmf_tile<unsigned, 0, 1, 5>);      // [yw]
  if (local) return f2d || packed || pair == LMF_PAIR5 || !ucf || !small ? LmfKernelRec{} : pair ? local_pairs : locals[yw];
  return packed ? packs[pair] : pair ? pairs[pair] : f2d ? plane[small] : six[yw][ucf][small];
}
static StrainKernelRec smag_rows_kernel(bool yw, bool small) {
  static const StrainKernelRec t[2][2] = {{KERNEL_REC(k_smag_rows<size_t, 0>), KERNEL_REC(k_smag_rows<unsigned, 0>)}, {KERNEL_REC(k_smag_rows<size_t, 1>), KERNEL_REC(k_smag_rows<unsigned, 1>)}};      // [yw][small]
  return t[yw][small];
}
// sgs_setup: the form, its flags, static kernel arguments and kernel records -- from the case, the switches and is_wall, before cales_create allocates the
// scratch fields of the form (pair fields or sij / mij)
void sgs_setup(cales_ctx *c) {
  SgsPath &P = c->sgs; const int *n = c->n; const Flags &fl = c->fl;
  if (c->C.sgstype == 0) return;
  bool xw = false, yw = false;      // the predicates, each computed here and nowhere else. Walls or wall model in x (the reference sequences only), in y
  for (int q = 0; q < 2; ++q) xw = xw || c->is_wall[q] != 0. || c->C.lwm[q] != 0;
  for (int q = 2; q < 4; ++q) yw = yw || c->is_wall[q] != 0. || c->C.lwm[q] != 0;
  const bool perx = CBP(c, 0, 1) == 'P' && CBP(c, 1, 1) == 'P' && !fl.dsmag_xghosts;      // x periodic and the kernels wrap around
  const bool perz = CBP(c, 0, 3) == 'P' && CBP(c, 1, 3) == 'P', zwalls = c->is_wall[4] != 0. && c->is_wall[5] != 0.;      // (walls: no-slip or wall-modelled)
  const bool small = (c->ntot + 16) * sizeof(real) < (1ull << 32) && !fl.wide_offsets;      // 32-bit byte offsets (ldb/stb)
  // the cell-centred velocity is not stored where the last pass can form it itself (k_lmf_tile<.., UCF = 1>): x periodic, z walls or periodic
  const bool ucf = perx && (zwalls || perz);
  const bool local = P.ave == SgsAve::local;      // a coefficient per cell: no cs(k) for the momentum pass to apply (lazy), and six components (five)
  if (c->C.sgstype == 1) P.form = !xw && n[2] >= 3 && n[1] >= 2 && !fl.smag_reference_sequence ? SgsForm::smag_rows : SgsForm::smag_reference;
  // (ducts: the fused last pass knows the wall rule along y from three rows on)
  else if (P.ave == SgsAve::xlines) P.form = SgsForm::dsmag_reference;      // (no tile form yet: k_lmf_tile hands out plane partials, not rows')
  else if (local && P.filter2d) P.form = SgsForm::dsmag_reference;      // (k_lmf_plane_tile has no local form)
  // local: the tile form where a LOCAL instantiation is built (lmf_kernel: ucf, 32-bit byte offsets); every other class, and a field beyond 4 GB, takes the sequence
  else if (local && !(ucf && small)) P.form = SgsForm::dsmag_reference;
  else if (!P.filter2d) P.form = !xw && !(yw && n[1] < 3) && n[2] >= 3 && !fl.dsmag_reference_sequence ? SgsForm::dsmag_tiles : SgsForm::dsmag_reference;
  // the plane filter (-D_FILTER_2D): tiles for the channel class -- ucf (the kernels wrap around in x, z between two walls or periodic) and nothing at the y
  // faces; every other case takes the sequence
  else P.form = ucf && !xw && !yw && n[2] >= 3 && !fl.dsmag_reference_sequence ? SgsForm::dsmag_tiles : SgsForm::dsmag_reference;
  P.wraps_x = P.form == SgsForm::smag_rows || (P.form == SgsForm::dsmag_tiles && !fl.dsmag_xghosts);
  if (P.form != SgsForm::smag_rows && P.form != SgsForm::dsmag_tiles) return;
  const bool smag = P.form == SgsForm::smag_rows;
  P.zlo = c->is_wall[4] != 0.; P.zhi = c->is_wall[5] != 0.;
  // wall-model faces in z: the strain rates see ghost planes extrapolated from the interior (extrapolate(...,lwm) with the
  // grid factor, sgs.f90:683-748) instead of the stress-carrying ghost cells
  P.wmlo = ISB(c, 0, 3) && LWM(c, 0, 3) != 0; P.wmhi = ISB(c, 1, 3) && LWM(c, 1, 3) != 0;
  P.flo = (1. / c->dzci[0]) * c->dzci[1]; P.fhi = (1. / c->dzci[n[2]]) * c->dzci[n[2] - 1];
  // y walls of a duct: dsmag on the rank that owns them (wall rule of the filters along y); smag_rows all of the case (van Driest distances use global
  // rows, the shear of both walls reaches every slab). Wall-model y faces: extrapolated ghost rows for the strain rates
  P.wylo = (smag || ISB(c, 0, 2)) && c->is_wall[2] != 0.; P.wyhi = (smag || ISB(c, 1, 2)) && c->is_wall[3] != 0.;
  P.wmylo = ISB(c, 0, 2) && LWM(c, 0, 2) != 0; P.wmyhi = ISB(c, 1, 2) && LWM(c, 1, 2) != 0;
  const bool ywk = P.wylo || P.wyhi || P.wmylo || P.wmyhi;      // the y logic of the kernels (YW)
  if (smag) { P.smag.k = smag_rows_kernel(ywk, small); return; }
  P.lazy = !local; for (int q = 0; q < 6; ++q) P.lazy = P.lazy && c->C.bcsgs[q] == 0.;
  P.perz = perz; P.perx = perx; P.ucf = ucf; P.skipz = zwalls ? 4 : 0;
  // |S|Sij as three fields of pairs between K_AC and the fused last pass: ucf, and y periodic (the one-launch ghost-cell kernel takes a pair field as a
  // field of twice the width), 32-bit byte offsets still enough for a field twice as long
  P.pair = !P.filter2d && ucf && CBP(c, 0, 2) == 'P' && CBP(c, 1, 2) == 'P' && !fl.wide_offsets && !fl.unmerged_bc && (2 * c->ntot + 64) * sizeof(real) < (1ull << 32);
  // five |S|Sij instead of six wherever the strain-rate pass projects the velocity itself (make_plan: fold_correc needs pair fields) on one rank -- on slabs the
  // scratch rows travel in counted planes and keep six
  P.five = P.pair && c->P == 1 && !fl.sgs_six_components && !local;
  // the remainder x tile packed into full waves (sgs_setup_launches): pair fields on one rank (local: no block sums, another instantiation)
  P.lmf_packed = P.pair && !local && c->P == 1 && lmf_pack(n[0]).on && !fl.lmf_unpacked_remainder;
  P.lmf_ty = ywk ? TYL : TYLF;
  // the passes (plane filter: ucf, no yw -- the form's condition)
  auto lmf = [&](int pair, bool packed) { return lmf_kernel(P.filter2d, pair, local, packed, ywk, ucf, small); };
  P.strain.k = strain_kernel(P.pair, P.filter2d, ywk, small); P.lmf[0].k = lmf(P.pair ? LMF_PAIR : 0, false);
  if (P.pair) { P.corr[0][0].k = corr_strain_kernel(false, false); if (c->P > 1) P.corr[1][0].k = corr_strain_kernel(true, false); }
  if (P.five) { P.corr[0][1].k = corr_strain_kernel(false, true); P.lmf[1].k = lmf(LMF_PAIR5, false); }
  if (P.lmf_packed) { P.lmf_rem[0].k = lmf(LMF_PAIR, true); if (P.five) P.lmf_rem[1].k = lmf(LMF_PAIR5, true); }
}
// sgs_setup_launches: the launch geometry of the tile passes (after cales_create has read the CU count: balanced_kchunk)
int sgs_setup_launches(cales_ctx *c) {
  SgsPath &P = c->sgs; const int *n = c->n;
  if (P.form == SgsForm::smag_rows) {
    // row-marching form: one wave per row of 62 cells; chunks of k so that every CU holds several blocks' worth of independent waves (the LDS-tile
    // form of this pass -- two barriers per plane, 2.4 against 2.9 TB/s -- lost its A/B in round 2 and went in round 4)
    const int rgx = (n[0] + 61) / 62, rgy = (n[1] + SROWS - 1) / SROWS;
    int kr = n[2];
    // sixteen waves per CU at a time: enough blocks for eight rounds or more, or the last round's idle CUs show (chunks pay a three-plane prologue)
    while ((long)rgx * rgy * ((n[2] + kr - 1) / kr) < 8192 && kr > 32) kr = (kr + 1) / 2;
    while ((long)rgx * rgy * ((n[2] + kr - 1) / kr) < 1024 && kr > 8) kr = (kr + 1) / 2;
    if (c->fl.kchunk > 0) kr = c->fl.kchunk < n[2] ? c->fl.kchunk : n[2];
    TileGeom &s = P.smag.geo; s.kchunk = kr; s.bm = band_map(rgx, rgy, (n[2] + kr - 1) / kr);
    s.block = dim3(64, SROWS, 1); s.grid = dim3(band_blocks(s.bm), 1, 1);
  }
  if (P.form != SgsForm::dsmag_tiles) return 0;
  // a missing kernel is an error, never another path: only LOCAL has instantiations that are not built (lmf_kernel), and sgs_setup must not take the tile form there
  if (!P.lmf[0].k.fn) { c->err = "dsmag: no local form of this last pass"; return 1; }
  // K_AC: tiles of 64 x TYS, folded 64 x TYC (with two ghost rows of the prediction on several slabs: two rows more); the last pass 62 x lmf_ty
  P.strain.geo = with_bands(tile_geom(c, TYS, 64));
  if (P.pair) { P.corr[0][0].geo = P.corr[0][1].geo = with_bands(tile_geom(c, TYC, 64)); P.corr[1][0].geo = with_bands(tile_geom(c, TYC, 64, 2)); }
  TileGeom t = tile_geom(c, P.lmf_ty, 62, 0, LMF_KMAX), rem;
  // The remainder x tile packed into full waves (lmf_pack.hpp; pair fields on one rank): the launch above keeps the full tiles, with the chunk length their
  // block count gives, and a launch of the packed instantiation takes the remainder tile of S y tiles per block, its chunk length from the same cost model
  // (few blocks: one round of short chunks). 512^3: 8 x 64 x 4 blocks -- eight full rounds of the 256 CUs instead of nine with every ninth block three
  // quarters dead lanes -- and 22 x 11 packed blocks of 47 planes. Every y tile's remainder sum keeps the slot it has in the one launch (lmf_gx x tiles per
  // row), so k_plane_fold adds the same numbers in the same order; a packed block keeps the sums of its S stretches' chunks in the LDS of one chunk of LMF_KMAX.
  P.lmf_gx = t.grid.x;
  if ((size_t)2 * n[2] * t.grid.x * t.grid.y > c->ntot) { c->err = "dsmag: partial-sum scratch too small"; return 1; }
  auto cap = [&](TileGeom &s, int kmax) { while (s.kchunk > kmax) { s.kchunk = (s.kchunk + 1) / 2; s.grid.z = (n[2] + s.kchunk - 1) / s.kchunk; } };      // the kernel keeps a chunk's block sums in LDS
  if (P.lmf_packed) {
    const LmfPack pk = lmf_pack(n[0]); const int gy = t.grid.y, kmax_rem = LMF_KMAX / pk.S;
    t.grid = dim3(pk.full, gy, 1); tile_chunks(c, t, LMF_KMAX);
    rem = t; rem.grid = dim3(1, lmf_pack_blocks(pk, gy), 1); tile_chunks(c, rem, kmax_rem); cap(rem, kmax_rem);
  }
  cap(t, LMF_KMAX);
  P.lmf[0].geo = P.lmf[1].geo = t; P.lmf_rem[0].geo = P.lmf_rem[1].geo = rem;
  return 0;
}
// the static wall arguments of a tile pass: the ten that StrainTileArgs and LijMijArgs both carry
template <typename A> static void wall_args(const SgsPath &P, A &a) {
  a.zlo = P.zlo; a.zhi = P.zhi; a.wmlo = P.wmlo; a.wmhi = P.wmhi; a.flo = P.flo; a.fhi = P.fhi;
  a.wylo = P.wylo; a.wyhi = P.wyhi; a.wmylo = P.wmylo; a.wmyhi = P.wmyhi;
}
// ---- the tile form of the dynamic model, in four steps (dsmag_fast below). What a call decides: fold (the projection of this substep is pending), and with it s12 != nullptr:
// FIVE components -- S12 as a plain field in the buffer of the pair field (S33,S12), placed like every field: cell (1, j, k) at the head of a 128-B line (field_alloc: a pair
// field starts 2 field_ofs reals into its allocation, a field field_ofs; 8 bytes off, every wave's 512-B store touches a fifth line).
// 1. K_AC: |S|, |S|Sij, cell-centred and test-filtered velocity in one pass over u,v,w (no wall-model faces -> extrapolate(...,lwm) is a no-op; u,v
// are extrapolated through the z walls, w on the faces is not, sgs.f90:705-710); fold (pair fields, make_plan): with the projection folded in, rows2:
// from two ghost rows of the prediction, forming the ghost rows of its outputs too
static int dsmag_strain_pass(cales_ctx *c, const SgsFold *fold, real *s12) {
  const SgsPath &P = c->sgs; const int *n = c->n; real **f = c->f;
  const bool ext = fold && fold->rows2;
  { ProfScope ps(c, fold ? "correc_strain_filter_uvw" : "strain_filter_uvw");
    const TilePass<StrainTileArgs> &pass = !fold ? P.strain : P.corr[ext][s12 != nullptr]; const TileGeom &t = pass.geo;
    StrainTileArgs S;
    S.u[0] = f[CALES_U]; S.u[1] = f[CALES_V]; S.u[2] = f[CALES_W]; S.s0 = P.lazy ? f[CALES_VISCT] : c->s0;
    for (int m = 0; m < 6; ++m) S.ssij[m] = c->sij[m];
    for (int m = 0; m < 3; ++m) S.ss2[m] = reinterpret_cast<real2 *>(c->ss2[m]);
    if (s12) S.ss2[1] = reinterpret_cast<real2 *>(s12);
    S.uc[0] = P.ucf ? nullptr : c->uc; S.uc[1] = P.ucf ? nullptr : c->vc; S.uc[2] = P.ucf ? nullptr : c->wc; S.uf[0] = c->uf; S.uf[1] = c->vf; S.uf[2] = c->wf;
    S.dzci = c->d_dzci; S.dzfi = c->d_dzfi; S.dxi = c->dli[0]; S.dyi = c->dli[1]; S.kchunk = t.kchunk;
    wall_args(P, S); S.twy = nullptr; S.dl2 = c->dl[1]; S.bm = t.bm; S.perx = c->step_xskip ? 1 : 0;
    if (fold) {      // corrected velocity on load, u, v, w to the second buffers, p += pp
      S.pp = f[CALES_PP]; S.p = f[CALES_P]; for (int q = 0; q < 3; ++q) S.un[q] = c->f2[q];
      S.force = c->d_force; S.fmask = fold->fmask;
      S.cdt = fold->dtrk; S.cfi = fold->dtrk * c->dli[0]; S.cfj = fold->dtrk * c->dli[1]; S.zper = P.perz;
      S.pery = c->P == 1 ? 1 : 0; S.ppd = c->pp_companion_bytes;
      const size_t pl = (size_t)(n[0] + 2) * (n[1] + 2);
      S.bcz[0][0] = c->bcu.z; S.bcz[0][1] = c->bcu.z + pl; S.bcz[1][0] = c->bcv.z; S.bcz[1][1] = c->bcv.z + pl;
      S.vcg = c->vc;
    }
    LAUNCH_REC(c, pass.k, t.grid, t.block, 0, c->stream, c->g, S); }
  if (!fold) return 0;
  // the corrected velocity sits in the second buffers: swap (as the fused momentum pass does), give the normal component its two z faces -- the
  // reference's correc covers w(:,:,0) (correc.f90:60-66) and leaves w(:,:,n3+1) as it was, and bounduvw with is_correc touches neither -- and
  // fill the ghost cells of u, v, w and p (the pressure rides along: pair fields come with the one-launch ghost-cell kernel) as main.f90:500-504
  // does after correc / updatep
  for (int q = 0; q < 3; ++q) std::swap(c->f[CALES_U + q], c->f2[q]);
  if (!P.perz)
    LAUNCH(c, k_wface_fold, dim3((n[0] + 2 + 63) / 64, (n[1] + 2 + 3) / 4), dim3(64, 4), 0, c->stream, c->g, c->f2[2], c->f[CALES_W], f[CALES_PP], fold->dtrk * c->dzci[0]);
  // several slabs: the ghost rows of u, v, w and p do not travel at all -- k_fold_ghost_rows forms them from the prediction's ghost rows and pp's,
  // the ghost-cell kernel below gives them their x and z ghost cells (round 5: in the same exchange as the scratch fields', fifteen planes; now eleven)
  if (c->P > 1 && !ext)      // (ext: the strain-rate pass has formed them itself)
    LAUNCH(c, k_fold_ghost_rows, dim3((n[0] + 63) / 64, (n[2] + 3) / 4, 2), dim3(64, 4), 0, c->stream, c->g, c->f2[0], c->f2[1], c->f2[2], c->f[CALES_U], c->f[CALES_V],
           c->f[CALES_W], f[CALES_PP], c->scr2, f[CALES_P], c->d_force, fold->fmask, fold->dtrk * c->dli[0], fold->dtrk * c->dli[1], fold->dtrk, c->d_dzci, c->step_xskip ? 1 : 0);
  BcCall bc; bc.rows_current = c->P > 1; bc.rider(f[CALES_P], 0);
  return op_bounduvw(c, VelSet::state, 1, 1, bc);
}
// 2. The ghost cells of the scratch fields, sgs-type: only the periodic exchange matters (products of ghosts = ghosts of products; the wall ghosts are
// replaced by the extrapolation rule inside the filters). The tile kernels alone read these fields: with periodic x their ghost columns are not filled
// (perx: the kernels wrap around instead; an x ghost update touches four cache lines per row for two values), and the z ghost planes of the quantities the
// wall rule covers are never read (skipz). Several ranks: ONE exchange for the y-halo rows of all these fields (six |S|Sij, three filtered velocities, v_c,
// and |S| itself in the lazy form inside cales_step) instead of one per ghost-cell call; their ghost-cell kernels run first, the rows that then arrive
// carry the neighbour's x/z ghost cells. overlap: on the second stream, beside the interior tiles of the last pass
static int dsmag_scratch_ghosts(cales_ctx *c, bool ext, real *s12, bool overlap, bool *visct_ghosts_done) {
  const SgsPath &P = c->sgs; const int *n = c->n; real **f = c->f;
  const bool five = s12 != nullptr;
  HaloBatch rows;
  BcCall bc; bc.skip = P.perx | P.skipz;
  if (ext) bc.rows_current = true;      // the ghost rows of every field below were formed by the strain-rate pass: their x and z ghost cells only
  else if (c->P > 1) bc.collect = &rows;
  BcCall bz = bc; bz.skip = P.perx;      // (the filtered velocity: its z ghost planes are read)
  // (five components: the pair fields (S11,S22) and (S13,S23); S12, a plain field at the head of ss2[1], goes with v_c below -- no launch more)
  real *ssp[3] = {c->ss2[0], five ? c->ss2[2] : c->ss2[1], c->ss2[2]};
  if (int e = P.pair ? op_boundp_wide(c, five ? 2 : 3, ssp, 1, bc) : op_boundp_multi(c, 6, c->sij, 1, bc)) return e;
  if (int e = op_bounduvw(c, VelSet::filtered, 0, 0, bz)) return e;
  if (!P.ucf) { real *cc[3] = {c->uc, c->vc, c->wc}; if (int e = op_boundp_multi(c, 3, cc, 1, bc)) return e; }
  else if (ext) { if (int e = op_boundp(c, c->vc, 1, bc)) return e; }      // (v_c of the two ghost rows came from the strain-rate pass)
  else if (!(P.wylo && P.wyhi)) {      // v_c of the rows 1 and n2 only: their copies in the ghost rows (periodic wrap or the slab neighbours') are what the last pass reads for row 0
    LAUNCH(c, k_vc_edge_rows, dim3((n[0] + 2 + 63) / 64, (n[2] + 2 + 3) / 4), dim3(64, 4), 0, c->stream, c->g, f[CALES_V], c->vc);
    real *two[2] = {c->vc, s12};
    if (int e = op_boundp_multi(c, five ? 2 : 1, two, 1, bc)) return e; }
  if (P.lazy && visct_ghosts_done && c->P > 1) {      // inside cales_step |S| is final (K_AC wrote it): its rows travel along
    BcCall bv = bc; bv.skip = 0;
    if (int e = op_boundp(c, f[CALES_VISCT], 1, bv)) return e;
    *visct_ghosts_done = true; }
  return halo_flush(c, rows, overlap);
}
// 3. K_B + K_DF in one pass: filter(|S|Sij) on the fly, strain rate of the filtered velocity, Mij, Lij, contractions, plane partial sums (local: visct itself)
static int dsmag_last_pass(cales_ctx *c, real *s12, bool overlap) {
  const SgsPath &P = c->sgs; const int *n = c->n; real **f = c->f;
  const bool five = s12 != nullptr;
  ProfScope ps(c, "lij_mij_filter_contract");
  const TilePass<LmfArgs> &pass = P.lmf[five]; const TileGeom &t = pass.geo;
  LmfArgs B; LijMijArgs &L = B.L;
  L.uc[0] = P.ucf ? f[CALES_U] : c->uc; L.uc[1] = P.ucf ? f[CALES_V] : c->vc; L.uc[2] = P.ucf ? f[CALES_W] : c->wc; L.uf[0] = c->uf; L.uf[1] = c->vf; L.uf[2] = c->wf;
  L.vcg = c->vc; L.perz = P.perz; L.xwrap = c->step_xskip ? 1 : 0;
  for (int m = 0; m < 6; ++m) L.mf[m] = c->mij[m];
  L.part = c->wk[0]; L.dzci = c->d_dzci; L.dzfi = c->d_dzfi; L.dxi = c->dli[0]; L.dyi = c->dli[1];
  wall_args(P, L); L.perx = P.perx;
  if (P.ave == SgsAve::local) { L.mf[0] = c->s0; L.part = f[CALES_VISCT]; }      // the pass writes visct itself, from |S| (never lazy: K_AC left it in c->s0)
  L.kchunk = t.kchunk; L.nblk = P.lmf_gx * t.grid.y; B.gx = P.lmf_gx;
  for (int m = 0; m < 6; ++m) B.ss[m] = c->sij[m];
  for (int m = 0; m < 3; ++m) B.ss2[m] = reinterpret_cast<const real2 *>(c->ss2[m]);
  if (five) B.ss2[1] = reinterpret_cast<const real2 *>(s12);
  auto launch = [&](int by0, int nby) {      // the y tiles by0 .. by0 + nby - 1
    if (nby <= 0) return;
    TileGeom s = t; s.grid.y = nby; s = with_bands(s);
    if (P.lmf_packed && c->fl.lmf_main_bands && !s.bm.gx) { s.bm = band_map(s.grid.x, s.grid.y, s.grid.z); s.grid = dim3(band_blocks(s.bm), 1, 1); }      // (experiments)
    B.by0 = by0; B.bm = s.bm;
    LAUNCH_REC(c, pass.k, s.grid, s.block, 0, c->stream, c->g, B);
  };
  if (overlap) {
    // several ranks with the second stream: tiles that read the ghost rows j = 0 or j = n2+1 wait for the rows in flight; the others run beside the exchange
    int hi0 = (int)t.grid.y; while (hi0 > 1 && (hi0 - 1) * P.lmf_ty + P.lmf_ty + 1 >= n[1] + 1) --hi0;      // first tile (> 0) that reaches row n2+1
    launch(1, hi0 - 1);
    if (int e = stream_after(c, c->stream, c->comm_stream)) return e;
    launch(0, 1); launch(hi0, (int)t.grid.y - hi0);
  } else launch(0, (int)t.grid.y);
  if (P.lmf_packed) {      // the remainder x tile of every row, S y tiles per block: its own chunk length, its block sums behind the others'
    const TilePass<LmfArgs> &rem = P.lmf_rem[five];
    LmfArgs R = B; R.L.kchunk = rem.geo.kchunk; R.by0 = 0; R.bm = BandMap{0, 0, 0, 0};
    LAUNCH_REC(c, rem.k, rem.geo.grid, rem.geo.block, 0, c->stream, c->g, R);
  }
  return 0;
}
// 4. (and the end of the reference sequence) The coefficient from the sums of MijLij and MijMij over the planes, and the eddy viscosity (sgs.f90:359-379). nblk
// != 0: the sums are still the nblk block sums per plane the last pass left in wk[0] -- folded in a fixed order first. s0: where |S| sits (not lazy)
static int dsmag_coefficient(cales_ctx *c, int nblk, const real *s0) {
  const SgsPath &P = c->sgs; const int *n = c->n; real *visct = c->f[CALES_VISCT];
  if (nblk) LAUNCH(c, k_plane_fold, dim3(2 * n[2]), dim3(256), 0, c->stream, n[2], nblk, c->wk[0], c->d_p1d);
  if (c->P > 1) { if (int e = allreduce_dev(c, c->d_p1d, 2 * n[2], 0)) return e; }   // sgs.f90:475
  if (P.ave == SgsAve::volume) LAUNCH(c, k_volume_fold, dim3(1), dim3(256), 0, c->stream, n[2], c->d_dzf, c->d_p1d);      // sgs.f90:360-361
  const real gar = c->dl[0] * c->dl[1] / (c->C.l[0] * c->C.l[1]);
  if (P.lazy) {      // |S| is in visct already: cs(k) alone, the momentum pass applies it
    if (!c->d_cs && ctx_alloc(c, &c->d_cs, n[2] + 2, false)) return 1;
    LAUNCH(c, k_dsmag_coef, dim3(1), dim3(256), 0, c->stream, n[2], gar, c->d_p1d, c->d_cs, P.perz);
    c->visct_lazy = true;
  } else { const dim3 b(BX, BY, 1); LAUNCH(c, k_dsmag_final, grid3(n[0], n[1], n[2], b), b, 0, c->stream, c->g, gar, c->d_p1d, s0, visct); }
  LAUNCHCHK(c);
  return 0;
}
static int dsmag_fast(cales_ctx *c, const SgsFold *fold, bool *visct_ghosts_done) {
  const SgsPath &P = c->sgs;
  const bool ext = fold && fold->rows2;
  const bool five = fold && !ext && P.five;      // (the identity holds for the velocity this call projects, not for one it is handed)
  real *const s12 = five ? c->ss2[1] - c->field_ofs : nullptr;
  const bool overlap = c->comm.halo_second_stream && !ext;      // (ext: no row of the scratch fields travels)
  if (int e = dsmag_strain_pass(c, fold, s12)) return e;
  if (int e = dsmag_scratch_ghosts(c, ext, s12, overlap, visct_ghosts_done)) return e;
  if (int e = dsmag_last_pass(c, s12, overlap)) return e;
  if (P.ave == SgsAve::local) { LAUNCHCHK(c); return 0; }      // sgs.f90:368-377: visct is written -- no fold, no all-reduce, no final kernel
  return dsmag_coefficient(c, P.lmf_gx * (int)P.lmf[0].geo.grid.y, c->s0);
}

static inline dim3 lin_grid(size_t n) { size_t b = (n + 255) / 256; if (b > 4096) b = 4096; return dim3((unsigned)b); }

__global__ void k_smag_del(int n, real dl1, real dl2, const real *__restrict__ dzf, real *__restrict__ del) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k < n) del[k] = pow(dl1 * dl2 * dzf[k], 1. / 3.);       // the filter width depends on k only (sgs.f90:145)
}
// c->d_del, made by the first Smagorinsky pass that needs it
static int smag_del(cales_ctx *c) {
  if (c->d_del) return 0;
  if (ctx_alloc(c, &c->d_del, c->n[2] + 2, false)) return 1;
  LAUNCH(c, k_smag_del, dim3((c->n[2] + 2 + 63) / 64), dim3(64), 0, c->stream, c->n[2] + 2, c->dl[0], c->dl[1], c->d_dzf, c->d_del);
  return 0;
}
// sqrt(tau_w) of the two y walls as planes twy(side, k, i) for the van Driest damping of cells whose nearest wall is a y wall (sgs.f90:117-143,
// cases 3 and 4). One slab: straight from the fields. Several slabs: the walls belong to the first and the last slab, every other rank needs
// their shear too -- the reference stays within "two subdomains between two opposite walls" (sanity.f90:98-111) because its 2-D pencil grid
// can (initmpi.f90:230-259); y slabs cannot, so the owners fill their plane, everybody else zeros, and one sum over the slabs (x + 0 + ... + 0:
// exact) hands both planes to every rank. The planes sit at the head of the staging buffer A, which is free between two exchanges.
static int wall_shear_y_planes(cales_ctx *c, int wylo, int wyhi, const real **out) {
  const int *n = c->n;
  const size_t cnt = (size_t)2 * (n[2] + 2) * c->g.s1;
  real *twy = c->wk[0];
  if (c->P > 1) {
    if (!(twy = stage_borrow(c, (int64_t)cnt))) return 1;
    HIPCHK(c, hipMemsetAsync(twy, 0, cnt * sizeof(real), c->stream));
  } else if (cnt > c->ntot) { c->err = "smag: wall-shear scratch too small"; return 1; }
  const int lo = wylo && ISB(c, 0, 2) ? 1 : 0, hi = wyhi && ISB(c, 1, 2) ? 1 : 0;
  if (lo || hi)
    LAUNCH(c, k_wall_shear_y, dim3((n[0] + 63) / 64, (n[2] + 3) / 4), dim3(64, 4), 0, c->stream, c->g, c->f[CALES_U], c->f[CALES_W], c->visc, c->dli[1], lo, hi, twy, c->step_xskip ? 1 : 0);
  LAUNCHCHK(c);
  if (int e = allreduce_dev(c, twy, (int64_t)cnt, 0)) return e;
  *out = twy;
  return 0;
}
// Static Smagorinsky for cases without walls or wall model in x: strain rate and van Driest damping in one pass of the row-marching kernel,
// u,v,w -> visct (4 words/cell instead of the 20 of copy + extrapolate + strain + smag)
static int smag_fast(cales_ctx *c) {
  const SgsPath &P = c->sgs; real **f = c->f;
  if (int e = smag_del(c)) return e;
  StrainTileArgs S = {};
  S.u[0] = f[CALES_U]; S.u[1] = f[CALES_V]; S.u[2] = f[CALES_W]; S.visct = f[CALES_VISCT];
  S.dzci = c->d_dzci; S.dzfi = c->d_dzfi; S.dxi = c->dli[0]; S.dyi = c->dli[1];
  wall_args(P, S); S.dl2 = c->dl[1]; S.twy = nullptr;
  S.zc = c->d_zc; S.del = c->d_del; S.l3 = c->C.l[2]; S.visc = c->visc; S.perx = c->step_xskip ? 1 : 0;
  if (S.wylo || S.wyhi) { if (int e = wall_shear_y_planes(c, S.wylo, S.wyhi, &S.twy)) return e; }
  const TileGeom &t = P.smag.geo;
  S.kchunk = t.kchunk; S.bm = t.bm;
  LAUNCH_REC(c, P.smag.k, t.grid, t.block, 0, c->stream, c->g, S);
  LAUNCHCHK(c);
  return 0;
}
// The reference's sequence of the static model, kernel per loop (walls or wall model in x, degenerate grids, CALES_SMAG_REFERENCE_SEQUENCE)
static int smag_sequence(cales_ctx *c) {
  const int *n = c->n, if123[3] = {1, 2, 3}; const size_t nt = c->ntot; real **f = c->f, **wk = c->wk;
  const dim3 b(BX, BY, 1), gr = grid3(n[0], n[1], n[2], b);
  // wk(1:3) = u,v,w ; extrapolate at wall-model faces ; strain rate (sgs.f90:84-92) -- without the copies: the ghost cells of
  // u,v,w at the wall-model faces are replaced in place, kept in wk(1), and given back before anything else reads them
  real *uvw[3] = {f[CALES_U], f[CALES_V], f[CALES_W]};
  const size_t need = 6 * ((size_t)(n[1] + 2) * (n[2] + 2) + (size_t)(n[0] + 2) * (n[2] + 2) + (size_t)(n[0] + 2) * (n[1] + 2));
  if (need <= c->ntot) {
    if (int e = extrapolate(c, 3, uvw, if123, 0, wk[0], 0)) return e;
    if (int e = strain_rate(c, uvw[0], uvw[1], uvw[2], c->s0, nullptr)) return e;
    if (int e = extrapolate(c, 3, uvw, if123, 0, wk[0], 1)) return e;
  } else {            // degenerate grids: the copies of the reference
    LAUNCH(c, k_copy3, lin_grid(nt), dim3(256), 0, c->stream, nt, f[CALES_U], f[CALES_V], f[CALES_W], wk[0], wk[1], wk[2]);
    if (int e = extrapolate(c, 3, wk, if123, 0)) return e;
    if (int e = strain_rate(c, wk[0], wk[1], wk[2], c->s0, nullptr)) return e;
  }
  SmagArgs A; A.w0 = c->is_wall[0]; A.w1 = c->is_wall[1]; A.w2 = c->is_wall[2]; A.w3 = c->is_wall[3]; A.w4 = c->is_wall[4]; A.w5 = c->is_wall[5];
  A.dl1 = c->dl[0]; A.dl2 = c->dl[1]; A.l3 = c->C.l[2]; A.dxi = c->dli[0]; A.dyi = c->dli[1]; A.visc = c->visc;
  A.sumw = 0.; for (int q = 0; q < 6; ++q) A.sumw += c->is_wall[q];
  if (int e = smag_del(c)) return e;
  const real *twy = nullptr;      // several slabs: the shear of the y walls comes from the slabs that own them
  if (c->P > 1 && (c->is_wall[2] != 0. || c->is_wall[3] != 0.)) { if (int e = wall_shear_y_planes(c, c->is_wall[2] != 0., c->is_wall[3] != 0., &twy)) return e; }
  LAUNCH(c, k_smag, gr, b, 0, c->stream, c->g, A, c->d_zc, c->d_dzci, c->d_del, f[CALES_U], f[CALES_V], f[CALES_W], c->s0, f[CALES_VISCT], twy);
  LAUNCHCHK(c);
  return 0;
}
// The reference's sequence of the dynamic model, kernel per loop (sgs.f90:153-380): wk(1:3) = u,v,w ; extrapolate at wall-model faces ; strain rate (sgs.f90:173-181) ...
static int dsmag_sequence(cales_ctx *c) {
  const int *n = c->n, if123[3] = {1, 2, 3}; const size_t nt = c->ntot; real **f = c->f, **wk = c->wk; real *visct = f[CALES_VISCT];
  const dim3 b(BX, BY, 1), gr = grid3(n[0], n[1], n[2], b);
  LAUNCH(c, k_copy3, lin_grid(nt), dim3(256), 0, c->stream, nt, f[CALES_U], f[CALES_V], f[CALES_W], wk[0], wk[1], wk[2]);
  if (int e = extrapolate(c, 3, wk, if123, 0)) return e;
  real **sij = c->sij, **mij = c->mij, **lij = c->sij;
  if (int e = strain_rate(c, wk[0], wk[1], wk[2], c->s0, sij)) return e;
  LAUNCH(c, k_copy1, lin_grid(nt), dim3(256), 0, c->stream, nt, c->s0, visct);
  if (int e = op_boundp(c, c->s0, 1)) return e;
  for (int m = 0; m < 6; ++m) if (int e = op_boundp(c, sij[m], 1)) return e;
  CP6 csij; P6 pwk, pmij; CP6 cmij;
  for (int m = 0; m < 6; ++m) { csij.p[m] = sij[m]; pwk.p[m] = wk[m]; pmij.p[m] = mij[m]; cmij.p[m] = mij[m]; }
  LAUNCH(c, k_s0sij, lin_grid(nt), dim3(256), 0, c->stream, nt, c->s0, csij, pwk);
  const int if0[6] = {0, 0, 0, 0, 0, 0};
  // the reference's -D_FILTER_2D (sgs.f90:211-247,296-327): filter2d instead of filter3d, WITHOUT the extrapolate(...,cbc) calls in front of the filters, the
  // first filtered velocity from u, v, w themselves, and one filter ratio; everything else of the sequence is shared
  const bool f2d = c->sgs.filter2d;
  auto filter = [&](const real *p, real *pf) {
    if (f2d) LAUNCH(c, k_filter2d, gr, b, 0, c->stream, c->g, p, pf); else LAUNCH(c, k_filter3d, gr, b, 0, c->stream, c->g, p, pf);
  };
  if (!f2d) { if (int e = extrapolate(c, 6, wk, if0, 1)) return e; }
  for (int m = 0; m < 6; ++m) filter(wk[m], mij[m]);
  if (!f2d) {
    LAUNCH(c, k_copy3, lin_grid(nt), dim3(256), 0, c->stream, nt, f[CALES_U], f[CALES_V], f[CALES_W], wk[0], wk[1], wk[2]);
    if (int e = extrapolate(c, 3, wk, if123, 1)) return e;
  }
  filter(f2d ? f[CALES_U] : wk[0], c->uf);
  filter(f2d ? f[CALES_V] : wk[1], c->vf);
  filter(f2d ? f[CALES_W] : wk[2], c->wf);
  if (int e = op_bounduvw(c, VelSet::filtered, 0, 0)) return e;
  real *ff[3] = {c->uf, c->vf, c->wf};
  if (int e = extrapolate(c, 3, ff, if123, 0)) return e;
  if (int e = strain_rate(c, c->uf, c->vf, c->wf, c->s0, sij)) return e;
  if (f2d) LAUNCH(c, k_mij_a2, gr, b, 0, c->stream, c->g, pmij, (real)2.52, c->s0, csij);
  else LAUNCH(c, k_mij, gr, b, 0, c->stream, c->g, pmij, c->alph2, c->s0, csij);
  LAUNCH(c, k_interp, gr, b, 0, c->stream, c->g, f[CALES_U], f[CALES_V], f[CALES_W], c->uc, c->vc, c->wc);
  if (int e = op_boundp(c, c->uc, 1)) return e;
  if (int e = op_boundp(c, c->vc, 1)) return e;
  if (int e = op_boundp(c, c->wc, 1)) return e;
  LAUNCH(c, k_uiuj, lin_grid(nt), dim3(256), 0, c->stream, nt, c->uc, c->vc, c->wc, pwk);
  if (!f2d) { if (int e = extrapolate(c, 6, wk, if0, 1)) return e; }
  for (int m = 0; m < 6; ++m) filter(wk[m], lij[m]);
  real *cc[3] = {c->uc, c->vc, c->wc};
  if (!f2d) { if (int e = extrapolate(c, 3, cc, if0, 1)) return e; }
  filter(c->uc, c->uf);
  filter(c->vc, c->vf);
  filter(c->wc, c->wf);
  CP6 clij; for (int m = 0; m < 6; ++m) clij.p[m] = lij[m];
  if (c->sgs.ave == SgsAve::xlines) {      // sgs.f90:366-367: x is local to a y slab -- nothing to communicate
    LAUNCH(c, k_contract_lines, dim3((n[1] * n[2] + 3) / 4), dim3(256), 0, c->stream, c->g, cmij, clij, c->uf, c->vf, c->wf, wk[0]);
    LAUNCH(c, k_dsmag_final_lines, gr, b, 0, c->stream, c->g, c->dl[0] / c->C.l[0], wk[0], visct, visct);
    LAUNCHCHK(c); return 0;
  }
  if (c->sgs.ave == SgsAve::local) {      // sgs.f90:368-377: no average, no reduction, no collective -- one kernel in place of k_contract + k_plane_sum + k_dsmag_final
    LAUNCH(c, k_contract_local, gr, b, 0, c->stream, c->g, cmij, clij, c->uf, c->vf, c->wf, visct);
    LAUNCHCHK(c); return 0;
  }
  LAUNCH(c, k_contract, gr, b, 0, c->stream, c->g, cmij, clij, c->uf, c->vf, c->wf, wk[0], wk[1]);
  LAUNCH(c, k_plane_sum, dim3(n[2], 2), dim3(256), 0, c->stream, c->g, wk[0], wk[1], c->d_p1d);
  return dsmag_coefficient(c, 0, visct);      // (|S| sits in visct: k_copy1 above)
}

// the form of cmpt_sgs this context takes (cales_describe_plan): the record op_cmpt_sgs launches
const char *sgs_path_name(const cales_ctx *c) {
  static const char *names[] = {"none", "smag_rows", "smag_reference_sequence", "dsmag_tiles", "dsmag_reference_sequence"};      // (SgsForm order)
  if (c->sgs.filter2d) return c->sgs.form == SgsForm::dsmag_tiles ? "dsmag_tiles(filter2d)" : "dsmag_reference_sequence(filter2d)";
  return c->sgs.pair ? "dsmag_tiles(pair_fields)" : names[(int)c->sgs.form];
}
// cmpt_sgs: the first call's work, then the form sgs_setup chose
int op_cmpt_sgs(cales_ctx *c, const SgsFold *fold, bool *visct_ghosts_done) {
  const int *n = c->n;
  if (c->C.sgstype == 0) {           // 'none': visct = 0 once (sgs.f90:62-68)
    if (c->sgs_first) { c->sgs_first = false; HIPCHK(c, hipMemsetAsync(c->f[CALES_VISCT], 0, c->ntot * sizeof(real), c->stream)); c->visct_zero = true; }
    return 0;
  }
  c->visct_lazy = false;      // the field is rewritten from scratch
  ProfScope ps(c, c->C.sgstype == 1 ? "cmpt_sgs_smag" : "cmpt_sgs_dsmag");
  if (c->sgs_first) {
    c->sgs_first = false;
    if (c->C.sgstype == 2 && !c->sgs.filter2d)      // (the plane filter: 2.52 everywhere, sgs.f90:817-821 -- no field)
      LAUNCH(c, k_alph2, grid3(n[0] + 2, n[1] + 2, n[2] + 2, dim3(64, 4, 1)), dim3(64, 4, 1), 0, c->stream, c->g, c->is_wall[0], c->is_wall[1],
                         c->is_wall[2], c->is_wall[3], c->is_wall[4], c->is_wall[5], c->alph2);
  }
  if (c->sgs.form == SgsForm::dsmag_tiles) return dsmag_fast(c, fold, visct_ghosts_done);
  if (c->sgs.form == SgsForm::smag_rows) return smag_fast(c);
  return c->sgs.form == SgsForm::smag_reference ? smag_sequence(c) : dsmag_sequence(c);
}
