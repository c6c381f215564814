/*
 * fused_ref.c — CPU restatement of one D2Q9-BGK lattice step in the library's two arithmetics.
 *
 * TEST INFRASTRUCTURE ONLY (tests/fused_ref.py builds and wraps it).  What LBM_FLAG_FUSED_ARITH promises is a fixed
 * sequence of correctly rounded fused multiply-adds (include/lbm_d2q9.h, csrc/kernels/common.h relax_core_fused);
 * this file states that sequence with fmaf() so that the device's bits can be held to something that is not the
 * device.  mode 0 is the exact (unfused) arithmetic, which tests/test_fused_ref.py pins to the oracle bit for bit:
 * pull, rebound, acceleration and the sums are shared by both modes, so what is then left to trust in mode 1 is the
 * dozen lines of relax_fused().
 *
 * Build: gcc -std=c99 -O2 -ffp-contract=off (no contraction by the compiler: every fused operation is written out);
 * with -fopenmp the rows of a step are shared among threads, which changes no bit: a row's result does not depend on
 * another row's, and the per-row sums are added up in row order afterwards.
 *
 * State: `cells` is (ny, nx, 9) floats, direction k of cell (x, y) at ((y * nx) + x) * 9 + k, the grid periodic in
 * both directions.  Directions: 0 rest, 1 east, 2 north, 3 west, 4 south, 5 NE, 6 NW, 7 SW, 8 SE.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

enum { NDIR = 9 };

typedef struct cell_result {
  float f[NDIR];   /* relaxed populations */
  float msq;       /* squared momentum (not divided by the density) */
  float rinv;      /* 1 / density */
} cell_result;

/* moments shared by both arithmetics: plain float additions, left to right */
typedef struct moments { float rho, mx, my; } moments;

static moments moments_of(const float* t)
{
  moments m;
  m.rho = t[0];
  for (int k = 1; k < NDIR; k++) m.rho += t[k];
  m.mx = t[1] + t[5]; m.mx += t[8]; m.mx -= t[3]; m.mx -= t[6]; m.mx -= t[7];
  m.my = t[2] + t[5]; m.my += t[6]; m.my -= t[4]; m.my -= t[7]; m.my -= t[8];
  return m;
}

/* direction pairs (plus, minus) that share the projection m[i] of the momentum: east/west on mx, north/south on my,
 * NE/SW on mx + my, SE/NW on mx - my */
static const int plus_dir[4] = {1, 2, 5, 8};
static const int minus_dir[4] = {3, 4, 7, 6};
static const float weight[NDIR] = {4.0f / 9.0f, 1.0f / 9.0f, 1.0f / 9.0f, 1.0f / 9.0f, 1.0f / 9.0f,
                                   1.0f / 36.0f, 1.0f / 36.0f, 1.0f / 36.0f, 1.0f / 36.0f};

/* mode 0: every product and sum rounded on its own */
static void relax_exact(const float* t, float omega, cell_result* r)
{
  const moments mo = moments_of(t);
  const float m[4] = {mo.mx, mo.my, mo.mx + mo.my, mo.mx - mo.my};
  const float rho = mo.rho;
  const float rinv = 1.0f / rho;
  const float msq = mo.mx * mo.mx + mo.my * mo.my;
  const float h = 0.5f * rinv * 3.0f;
  float eq[NDIR];
  eq[0] = rho - h * msq;
  for (int i = 0; i < 4; i++) {
    const float a = m[i] * 3.0f;
    const float d = h * (a * m[i] - msq);
    eq[plus_dir[i]] = (rho + a) + d;
    eq[minus_dir[i]] = (rho - a) + d;
  }
  for (int k = 0; k < NDIR; k++) {
    const float q = weight[k] * eq[k];
    r->f[k] = t[k] + omega * (q - t[k]);
  }
  r->msq = msq;
  r->rinv = rinv;
}

/* mode 1: the fused sequence of LBM_FLAG_FUSED_ARITH; fmaf = one correctly rounded fused multiply-add */
static void relax_fused(const float* t, float omega, cell_result* r)
{
  const moments mo = moments_of(t);
  const float m[4] = {mo.mx, mo.my, mo.mx + mo.my, mo.mx - mo.my};
  const float rho = mo.rho;
  const float rinv = 1.0f / rho;
  const float msq = fmaf(mo.my, mo.my, mo.mx * mo.mx);
  const float h = 0.5f * rinv * 3.0f;
  float s[NDIR];
  s[0] = fmaf(-h, msq, rho);
  for (int i = 0; i < 4; i++) {
    const float a = m[i] * 3.0f;
    const float d = fmaf(a, m[i], -msq);
    s[plus_dir[i]] = fmaf(h, d, rho + a);
    s[minus_dir[i]] = fmaf(h, d, rho - a);
  }
  for (int k = 0; k < NDIR; k++) {
    const float q = fmaf(weight[k], s[k], -t[k]);
    r->f[k] = fmaf(omega, q, t[k]);
  }
  r->msq = msq;
  r->rinv = rinv;
}

/* the flow's driving force on one row: free cells whose westward populations stay positive */
static void accelerate_row(int nx, float density, float accel, float* row, const int* blocked)
{
  const float w1 = density * accel * 0.111111111111111111111111f;
  const float w2 = density * accel * 0.0277777777777777777777778f;
  for (int x = 0; x < nx; x++) {
    float* f = row + (size_t)x * NDIR;
    if (blocked[x]) continue;
    if (f[3] - w1 > 0.0f && f[6] - w2 > 0.0f && f[7] - w2 > 0.0f) {
      f[1] += w1; f[5] += w2; f[8] += w2;
      f[3] -= w1; f[6] -= w2; f[7] -= w2;
    }
  }
}

void fused_ref_init(int nx, int ny, float density, float* cells)
{
  const float w0 = density * 4.0f / 9.0f, w1 = density / 9.0f, w2 = density / 36.0f;
  for (size_t c = 0; c < (size_t)nx * (size_t)ny; c++) {
    float* f = cells + c * NDIR;
    f[0] = w0;
    for (int k = 1; k < 5; k++) f[k] = w1;
    for (int k = 5; k < NDIR; k++) f[k] = w2;
  }
}

/* msq and rinv of n cells given by their nine streamed-in populations t[c * 9 + k], as relax_exact (mode 0) or relax_fused
 * (mode 1) form them: what the velocity term of a cell is made of (tests/terms_ref.py). */
void fused_ref_cells(size_t n, const float* t, float omega, int mode, float* msq, float* rinv)
{
  for (size_t c = 0; c < n; c++) {
    cell_result r;
    if (mode) relax_fused(t + c * NDIR, omega, &r); else relax_exact(t + c * NDIR, omega, &r);
    msq[c] = r.msq;
    rinv[c] = r.rinv;
  }
}

static int run_impl(int nx, int ny, float density, float accel, float omega, const int* blocked, float* cells, int n_steps,
                    int mode, int nthreads, double* sums, double* terms);

/*
 * n_steps steps in place on `cells`.  Each step: acceleration of row ny - 2, then for every cell the pull from its
 * eight neighbours, rebound (blocked cells) or relaxation (the others), and the velocity term
 * sqrt((double)msq) * (double)rinv of every free cell, summed in double (a row at a time, then the rows) into
 * sums[step].  mode: 0 exact, 1 fused.  nthreads: threads sharing the rows (1 without OpenMP).  Returns 0, or -1 when
 * out of memory.
 */
int fused_ref_run(int nx, int ny, float density, float accel, float omega, const int* blocked, float* cells, int n_steps,
                  int mode, int nthreads, double* sums)
{
  return run_impl(nx, ny, density, accel, omega, blocked, cells, n_steps, mode, nthreads, sums, NULL);
}

/* ONE step of fused_ref_run that also hands out the velocity term of every cell: terms[y * nx + x], 0 at blocked cells. */
int fused_ref_step_terms(int nx, int ny, float density, float accel, float omega, const int* blocked, float* cells,
                         int mode, int nthreads, double* sum, double* terms)
{
  return run_impl(nx, ny, density, accel, omega, blocked, cells, 1, mode, nthreads, sum, terms);
}

static int run_impl(int nx, int ny, float density, float accel, float omega, const int* blocked, float* cells, int n_steps,
                    int mode, int nthreads, double* sums, double* terms)
{
  static const int reverse[NDIR] = {0, 3, 4, 1, 2, 7, 8, 5, 6};
  /* where direction k of a cell comes from: the neighbour at (x - dx[k], y - dy[k]) */
  static const int dx[NDIR] = {0, 1, 0, -1, 0, 1, -1, -1, 1};
  static const int dy[NDIR] = {0, 0, 1, 0, -1, 1, 1, -1, -1};
  const size_t n = (size_t)nx * (size_t)ny * NDIR;
  float* next = (float*)malloc(n * sizeof(float));
  double* row_totals = (double*)malloc((size_t)ny * sizeof(double));
  if (!next || !row_totals) { free(next); free(row_totals); return -1; }
  if (nthreads < 1) nthreads = 1;
  (void)nthreads;
  float* cur = cells;
  for (int step = 0; step < n_steps; step++) {
    accelerate_row(nx, density, accel, cur + (size_t)(ny - 2) * nx * NDIR, blocked + (size_t)(ny - 2) * nx);
#pragma omp parallel for schedule(static) num_threads(nthreads)
    for (int y = 0; y < ny; y++) {
      double row_total = 0.0;
      /* the rows below, at and above y (periodic) */
      const float* row[3] = {cur + (size_t)(y == 0 ? ny - 1 : y - 1) * nx * NDIR, cur + (size_t)y * nx * NDIR,
                             cur + (size_t)(y + 1 == ny ? 0 : y + 1) * nx * NDIR};
      for (int x = 0; x < nx; x++) {
        const int col[3] = {x == 0 ? nx - 1 : x - 1, x, x + 1 == nx ? 0 : x + 1};
        float t[NDIR];
        for (int k = 0; k < NDIR; k++) t[k] = row[1 - dy[k]][(size_t)col[1 - dx[k]] * NDIR + k];
        float* out = next + ((size_t)y * nx + x) * NDIR;
        if (blocked[(size_t)y * nx + x]) {
          for (int k = 0; k < NDIR; k++) out[reverse[k]] = t[k];
          if (terms) terms[(size_t)y * nx + x] = 0.0;
        } else {
          cell_result r;
          if (mode) relax_fused(t, omega, &r); else relax_exact(t, omega, &r);
          memcpy(out, r.f, sizeof r.f);
          const double term = sqrt((double)r.msq) * (double)r.rinv;
          row_total += term;
          if (terms) terms[(size_t)y * nx + x] = term;
        }
      }
      row_totals[y] = row_total;
    }
    double total = 0.0;
    for (int y = 0; y < ny; y++) total += row_totals[y];
    sums[step] = total;
    float* swap = cur; cur = next; next = swap;
  }
  if (cur != cells) {
    memcpy(cells, cur, n * sizeof(float));
    next = cur;
  }
  free(next);
  free(row_totals);
  return 0;
}
