/*
 * f64_ref.c — CPU restatement of the double-precision mode (include/lbm_d2q9_f64.h): the reference's lattice step with every
 * float object a double, every literal the same decimal read as a double, nothing contracted.
 *
 * TEST INFRASTRUCTURE ONLY (tests/f64_ref.py wraps it).  Build: gcc -std=c99 -O2 -ffp-contract=off [-fopenmp] -lm.
 *
 * Written from the contract in this repository's own words: a table of the nine lattice directions drives the pull, the
 * equilibrium and the bounce-back, one cell at a time on two AoS grids.  The kernels compute the same values by another route
 * (opposite directions share work, SoA planes, x-pairs), so agreement of the bits is agreement of two statements.  What must match
 * the reference is the ORDER of the floating-point operations of a cell (d2q9-bgk.c:546-666): each formula below says which.
 *
 * Rows are shared among threads; every per-step sum is formed from a stored array of terms by one thread in a fixed order, so the
 * thread count changes no bit.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define Q 9

/* direction k moves a population by (DX[k], DY[k]) per step (d2q9-bgk.c:26-36: 0 rest, 1 east, 2 north, 3 west, 4 south, 5 NE, 6 NW, 7 SW, 8 SE) */
static const int DX[Q] = {0, 1, 0, -1, 0, 1, -1, -1, 1};
static const int DY[Q] = {0, 0, 1, 0, -1, 1, 1, -1, -1};
static const int BACK[Q] = {0, 3, 4, 1, 2, 7, 8, 5, 6};          /* the direction opposite to k (:687-695) */

/* rest state (:880-902) */
void f64_ref_init(int nx, int ny, double density, double* cells)
{
  const double rest = density * 4.0 / 9.0, axis = density / 9.0, diag = density / 36.0;
  for (size_t c = 0; c < (size_t)nx * (size_t)ny; c++) {
    double* f = cells + c * Q;
    f[0] = rest;
    for (int k = 1; k < 5; k++) f[k] = axis;
    for (int k = 5; k < Q; k++) f[k] = diag;
  }
}

/* accelerate_flow on one free cell (:457-469) */
static void push_cell(double* f, double axis, double diag)
{
  if (f[3] - axis > 0.0 && f[6] - diag > 0.0 && f[7] - diag > 0.0) {      /* :457-460 */
    f[1] += axis; f[5] += diag; f[8] += diag;
    f[3] -= axis; f[6] -= diag; f[7] -= diag;
  }
}

/* the two weights of accelerate_flow (:445-446) */
void f64_ref_accel_weights(double density, double accel, double* axis, double* diag)
{
  *axis = density * accel * 0.111111111111111111111111;                   /* :445 */
  *diag = density * accel * 0.0277777777777777777777778;                  /* :446 */
}

/* accelerate_flow on one row (:442-478) */
static void push_row(int nx, double density, double accel, double* row, const int* blocked)
{
  double axis, diag;
  f64_ref_accel_weights(density, accel, &axis, &diag);
  for (int x = 0; x < nx; x++)
    if (!blocked[x]) push_cell(row + (size_t)x * Q, axis, diag);
}

/* One fluid cell: in[] = the nine populations that streamed in, out[] = after relaxation; returns sqrt(m^2) / rho (:667).
 * mom, where given, receives the density the cell had and its squared momentum. */
static double collide(const double* in, double omega, double* out, double* mom)
{
  static const double WEIGHT[Q] = {4.0 / 9.0, 1.0 / 9.0, 1.0 / 9.0, 1.0 / 9.0, 1.0 / 9.0, 1.0 / 36.0, 1.0 / 36.0, 1.0 / 36.0, 1.0 / 36.0};   /* :499-501 */
  double rho = 0.0;                                             /* :546-554: left to right from 0 */
  for (int k = 0; k < Q; k++) rho += in[k];
  const double rinv = 1.0 / rho;                                /* :561 */
  const double mx = in[1] + in[5] + in[8] - in[3] - in[6] - in[7];   /* :570-574, the momentum (never divided by rho) */
  const double my = in[2] + in[5] + in[6] - in[4] - in[7] - in[8];   /* :576-580 */
  const double msq = mx * mx + my * my;                         /* :589 */
  double along[Q];                                              /* :596-603: the momentum along each direction */
  along[0] = 0.0;
  along[1] = mx;       along[2] = my;       along[3] = -mx;      along[4] = -my;
  along[5] = mx + my;  along[6] = -mx + my; along[7] = -mx - my; along[8] = mx - my;
  const double half = 0.5 * rinv * 3.0;                         /* (0.5 * densinv) * ic_sq, the prefix of :638-646 */
  for (int k = 0; k < Q; k++) {
    double eq;
    if (k == 0) {
      eq = WEIGHT[0] * (rho - half * msq);                      /* :638 */
    } else {
      const double lin = along[k] * 3.0;                        /* :610-617 */
      const double quad = lin * along[k];                       /* :624-631 */
      eq = WEIGHT[k] * (rho + lin + half * (quad - msq));       /* :639-646 */
    }
    out[k] = in[k] + omega * (eq - in[k]);                      /* :658-666 */
  }
  if (mom) { mom[0] = rho; mom[1] = msq; }
  return sqrt(msq) * rinv;                                      /* :667 */
}

/* A cell after streaming: bounce-back (:687-695) where blocked, else collide(); returns the cell's term, 0.0 where blocked. */
static double finish(const double* in, int blocked, double omega, double* out, double* mom)
{
  if (blocked) {
    for (int k = 0; k < Q; k++) out[BACK[k]] = in[k];
    if (mom) mom[0] = mom[1] = 0.0;
    return 0.0;
  }
  return collide(in, omega, out, mom);
}

/*
 * n cells that have no neighbours: in[c] = the nine populations that streamed into cell c.  out[c] = after bounce-back or relaxation
 * and, where accel[c] is set and the cell is free, after the NEXT step's accelerate_flow with the weights w1 (axis) and w2 (diagonal):
 * what a kernel that fuses that pre-pass into its epilogue stores.  term[c] = the cell's term, 0.0 where blocked.
 */
static void cells_each(size_t n, const double* in, const int* blocked, const int* accel, double omega, double w1, double w2, double* out,
                       double* term, double* mom)
{
  for (size_t c = 0; c < n; c++) {
    term[c] = finish(in + c * Q, blocked[c], omega, out + c * Q, mom ? mom + 2 * c : NULL);
    if (accel[c] && !blocked[c]) push_cell(out + c * Q, w1, w2);
  }
}

void f64_ref_cells(size_t n, const double* in, const int* blocked, const int* accel, double omega, double w1, double w2, double* out, double* term)
{
  cells_each(n, in, blocked, accel, omega, w1, w2, out, term, NULL);
}

/* f64_ref_cells, and mom[c] = {the density, the squared momentum} collide() formed for cell c (zeros where blocked): what the tests
 * count to show which regimes their inputs reach. */
void f64_ref_cells_moments(size_t n, const double* in, const int* blocked, const int* accel, double omega, double w1, double w2, double* out,
                           double* term, double* mom)
{
  cells_each(n, in, blocked, accel, omega, w1, w2, out, term, mom);
}

enum { F64_REF_POSITIVE = 1, F64_REF_NAN_TERM = 2, F64_REF_POS_INF_TERM = 4, F64_REF_NEG_INF_TERM = 8 };

static int wrap(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

/* Neumaier's compensated sum in long double: the terms' exactly rounded sum for every count a test uses */
static double sum_exact(const double* v, size_t n)
{
  long double s = 0.0L, comp = 0.0L;
  for (size_t i = 0; i < n; i++) {
    const long double x = v[i], t = s + x;
    if (fabsl(s) >= fabsl(x)) comp += (s - t) + x;
    else comp += (x - t) + s;
    s = t;
  }
  return (double)(s + comp);
}

static double sum_rows(const double* term, int nx, int y0, int y1)
{
  double s = 0.0;
  for (int y = y0; y < y1; y++)
    for (int x = 0; x < nx; x++) s += term[(size_t)y * nx + x];
  return s;
}

/*
 * n_steps steps on cells (ny*nx*9 doubles, in place).  Per step t:
 *   serial[t] = the sum of the free cells' terms as the reference adds them with one rank (:350,365-366): rows 1..ny-2 into one
 *               accumulator, row 0 into a second, row ny-1 into a third, then first + second + third;
 *   exact[t]  = their exactly rounded sum.
 * Neither is divided by the number of free cells.  Blocked cells contribute the term 0.0 to both (x + 0.0 == x).
 * Returns 0, or -1 when out of memory.
 */
static int run_steps(int nx, int ny, double density, double accel, double omega, const int* blocked, double* cells, int n_steps, int nthreads,
                     double* serial, double* exact, int* status, double* abs_exact)
{
  const size_t n = (size_t)nx * (size_t)ny;
  double* next = (double*)malloc(sizeof(double) * n * Q);
  double* term = (double*)malloc(sizeof(double) * n);
  double* mom = status ? (double*)malloc(sizeof(double) * n * 2) : NULL;      /* {density, squared momentum} per cell */
  double* mag = status ? (double*)malloc(sizeof(double) * n) : NULL;          /* |term| per cell */
  double* cur = cells;
  if (!next || !term || (status && (!mom || !mag))) { free(next); free(term); free(mom); free(mag); return -1; }
  if (nthreads < 1) nthreads = 1;
  (void)nthreads;
  for (int t = 0; t < n_steps; t++) {
    push_row(nx, density, accel, cur + (size_t)(ny - 2) * nx * Q, blocked + (size_t)(ny - 2) * nx);     /* :345-348, :449 */
#ifdef _OPENMP
#pragma omp parallel for schedule(static) num_threads(nthreads)
#endif
    for (int y = 0; y < ny; y++) {
      const size_t from_row[3] = {(size_t)wrap(y - 1, ny) * nx, (size_t)y * nx, (size_t)wrap(y + 1, ny) * nx};   /* by 1 - DY[k] */
      for (int x = 0; x < nx; x++) {
        const size_t c = (size_t)y * nx + x;
        const size_t from_col[3] = {(size_t)wrap(x - 1, nx), (size_t)x, (size_t)wrap(x + 1, nx)};               /* by 1 - DX[k] */
        double in[Q];
        for (int k = 0; k < Q; k++)                                                                     /* :526-538: from the cell at (x - DX, y - DY) */
          in[k] = cur[(from_row[1 - DY[k]] + from_col[1 - DX[k]]) * Q + k];
        term[c] = finish(in, blocked[c], omega, next + c * Q, mom ? mom + 2 * c : NULL);
      }
    }
    if (status) {
      int st = F64_REF_POSITIVE;
      for (size_t c = 0; c < n; c++) {
        mag[c] = fabs(term[c]);
        if (blocked[c]) continue;
        if (!(mom[2 * c] > 0.0)) st &= ~F64_REF_POSITIVE;
        if (isnan(term[c])) st |= F64_REF_NAN_TERM;
        else if (isinf(term[c])) st |= term[c] > 0.0 ? F64_REF_POS_INF_TERM : F64_REF_NEG_INF_TERM;
      }
      status[t] = st;
      abs_exact[t] = sum_exact(mag, n);
    }
    if (serial) {
      double s = sum_rows(term, nx, 1, ny - 1);
      s += sum_rows(term, nx, 0, 1);
      s += sum_rows(term, nx, ny - 1, ny);
      serial[t] = s;
    }
    if (exact) exact[t] = sum_exact(term, n);
    double* sw = cur; cur = next; next = sw;
  }
  if (cur != cells) { memcpy(cells, cur, sizeof(double) * n * Q); next = cur; }
  free(next);
  free(term);
  free(mom);
  free(mag);
  return 0;
}

int f64_ref_run(int nx, int ny, double density, double accel, double omega, const int* blocked, double* cells, int n_steps, int nthreads,
                double* serial, double* exact)
{
  return run_steps(nx, ny, density, accel, omega, blocked, cells, n_steps, nthreads, serial, exact, NULL, NULL);
}

/*
 * f64_ref_run, and per step what decides how a sum of that step's terms can be compared:
 *   status[t]     F64_REF_POSITIVE where every free cell had a positive density (with finite terms: every term non-negative, the premise
 *                 of the summation bounds the tests hold av_vels to); F64_REF_NAN_TERM, _POS_INF_TERM, _NEG_INF_TERM where some free
 *                 cell's term was a NaN, +inf, -inf;
 *   abs_exact[t]  the exactly rounded sum of the terms' magnitudes.
 * status and abs_exact are given together.
 */
int f64_ref_run_report(int nx, int ny, double density, double accel, double omega, const int* blocked, double* cells, int n_steps, int nthreads,
                       double* serial, double* exact, int* status, double* abs_exact)
{
  return run_steps(nx, ny, density, accel, omega, blocked, cells, n_steps, nthreads, serial, exact, status, abs_exact);
}
