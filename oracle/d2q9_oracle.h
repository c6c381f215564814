/*
 * d2q9_oracle.h — CPU restatement of the reference's D2Q9-BGK timestep path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under oracle/ is part of the product: only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library, and there only as
 * the checker / the reported CPU baseline.  The product path (mpilattice-boltzmann_amd/) never
 * links, imports or executes it.
 *
 * Parity status: PINNED.  `make -C oracle ref` compiles the unmodified reference
 * (/root/reference/d2q9-bgk.c) and tests/golden/make_fixtures.py checks that this restatement's
 * final_state.dat / av_vels.dat are byte-identical to the reference binary's on the four shipped
 * decks and on truncated / synthetic decks (digests committed in tests/golden/digests.json).
 *
 * Every function cites the reference lines it follows (paths relative to /root/reference/).
 * Cell storage here is the reference's AoS t_speed (d2q9-bgk.c:95-98): 9 floats per cell,
 * row-major, x fastest.  "Halo'd" arrays carry one extra row before and after the owned rows
 * (d2q9-bgk.c:248-251, 865-877).
 */
#ifndef D2Q9_ORACLE_H
#define D2Q9_ORACLE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORACLE_NSPEEDS 9

/* d2q9-bgk.c:79-90 (t_param) minus the derived free_cells_inv, which is carried separately. */
typedef struct oracle_params {
  int nx, ny, max_iters, reynolds_dim;
  float density, accel, omega;
} oracle_params;

/* d2q9-bgk.c:772-803.  Returns 0, or -1 with the reference's die() message in err. */
int oracle_read_params(const char* path, oracle_params* p, char* err, size_t errlen);

/* d2q9-bgk.c:917-953.  obstacles: ny*nx ints, zero-filled then marked; *free_cells as :805,945-946. */
int oracle_read_obstacles(const char* path, int nx, int ny, int* obstacles, int* free_cells,
                          char* err, size_t errlen);

/* d2q9-bgk.c:834-862 row decomposition.  ny_local/displs have `size` entries. */
void oracle_decompose(int ny, int size, int* ny_local, int* displs);

/* d2q9-bgk.c:880-902.  Fills `rows` rows of nx AoS cells. */
void oracle_init_cells(const oracle_params* p, float* cells, int rows);

/* d2q9-bgk.c:442-478 applied to ONE row of nx AoS cells with its nx obstacle flags. */
void oracle_accelerate_row(const oracle_params* p, float* row_cells, const int* row_obstacles);

/* d2q9-bgk.c:493-704 on a halo'd partition: cells/tmp_cells/obstacles have (rows+2)*nx entries,
 * owned rows are 1..rows; computes local rows [start,end) and returns their tot_u accumulated in
 * the reference's order and precision (float accumulator, double sqrt·rinv term, :667).
 * If terms != NULL it also receives the per-cell double term (0 for obstacle cells), indexed like
 * obstacles. */
float oracle_timestep_rows(const oracle_params* p, const float* cells, float* tmp_cells,
                           const int* obstacles, int start, int end, double* terms);

/* d2q9-bgk.c:707-757 without the MPI_Reduce: returns tot_u (float accumulator) over `rows` un-halo'd rows. */
float oracle_av_velocity_sum(const oracle_params* p, const float* cells, const int* obstacles, int rows);

/* d2q9-bgk.c:1002-1008 given av_velocity's result. */
float oracle_reynolds(const oracle_params* p, float av_velocity);

/* d2q9-bgk.c:1071-1119 for one cell: u_x,u_y,u,pressure as written to final_state.dat. */
void oracle_cell_observables(const oracle_params* p, const float* cell, int obstacle,
                             float* u_x, float* u_y, float* u, float* pressure);

/* Whole run = d2q9-bgk.c:315-396 for one rank (periodic self-exchange, :245-247), MPI-free.
 *   cells_out : ny*nx*9 floats, final state (un-halo'd AoS)
 *   av_vels   : max_iters floats, reference summation order (interior rows, row 0, row ny-1; :350,365-367)
 *   av_exact  : optional, max_iters doubles: same per-cell terms summed in double, row by row, times
 *               (double)free_cells_inv — order-insensitive yardstick for GPU tree reductions
 *   nthreads  : rows are split over this many OpenMP threads (1 = the reference's serial loop);
 *               results are identical for every nthreads.
 *   n_steps   : number of steps to run (<= max_iters; the reference always runs max_iters)
 * Returns 0. */
int oracle_run(const oracle_params* p, const int* obstacles, int free_cells, int n_steps,
               int nthreads, float* cells_out, float* av_vels, double* av_exact);

/* The exactly rounded sum of terms[c] over the n entries with obstacles[c] == 0 (obstacles == NULL: over all of them): the one
 * double nearest to the true sum, whatever the order — what math.fsum returns.  Finite terms.  Returns 0, or -1 out of memory. */
int oracle_exact_sum(const double* terms, const int* obstacles, size_t n, double* sum);

/* oracle_run with two more arguments:
 *   cells0    : optional, ny*nx*9 floats: the state the run starts from instead of the rest equilibrium
 *   sum_exact : optional, n_steps doubles: per step the exactly rounded sum over the free cells of the per-cell double terms
 *               (the terms av_exact adds row by row), NOT multiplied by free_cells_inv — the yardstick the device's
 *               per-step double sums are held to */
int oracle_run_sums(const oracle_params* p, const int* obstacles, int free_cells, int n_steps, int nthreads,
                    const float* cells0, float* cells_out, float* av_vels, double* av_exact, double* sum_exact);

/* Same loop, but without per-cell term storage and with a per-thread float accumulator: this is
 * the form timed as the CPU baseline (row-parallel, as BASELINE.md §4).  av_vels differ from
 * oracle_run's only in summation order when nthreads > 1; cells_out is identical. */
int oracle_run_fast(const oracle_params* p, const int* obstacles, int free_cells, int n_steps,
                    int nthreads, float* cells_out, float* av_vels);

/* d2q9-bgk.c:1049-1140 output formats.  displ = global index of row 0 of `cells`. */
int oracle_write_final_state(const char* path, const oracle_params* p, const float* cells,
                             const int* obstacles, int rows, int displ, int append);
int oracle_write_av_vels(const char* path, const float* av_vels, int n);

#ifdef __cplusplus
}
#endif
#endif
