/*
 * ref_sched.c -- runs the reference's time_dev kernel, compiled as C, under
 * one serialising schedule (TEST INFRASTRUCTURE ONLY).
 *
 * Every work-item is a ucontext fiber.  The work-groups run one after
 * another; inside a work-group the live work-items run in id order up to
 * their next barrier(), again and again until all have returned.  This is
 * the schedule the project's contract names ("one serialising runtime, one
 * work-group"); the arithmetic is the reference's own.
 */
#include <stdlib.h>
#include <ucontext.h>

#define REF_STACK (64 * 1024)

void time_dev(double *f, double *x, double *xx0, double *newf, double *newx, double *newxx0, double *omega,
              unsigned long *rand1, int *stable, const double *deltaTau, int *lrgEl, double *lrgVl, int *initRun,
              const int *LIST_SIZE, const double *deltaT, int *runs, const int *potential, const double *C,
              const int *Loops);

static ucontext_t g_sched;
static ucontext_t *g_fiber;
static char *g_done;
static void **g_args;
static int g_cur, g_base, g_global;

int get_global_id(int dim) { (void)dim; return g_base + g_cur; }
int get_global_size(int dim) { (void)dim; return g_global; }
void barrier(int flags) { (void)flags; swapcontext(&g_fiber[g_cur], &g_sched); }

static void fiber_main(void)
{
    void **a = g_args;
    time_dev(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15],
             a[16], a[17], a[18]);
    g_done[g_cur] = 1;
}

/* One NDRange of time_dev: `global` work-items in groups of `local`.
 * Returns 0, or -1 when the sizes are unusable or memory runs out. */
int ref_launch(void *args[19], int global, int local)
{
    if (global <= 0 || local <= 0 || global % local != 0) return -1;
    char *stacks = (char *)malloc((size_t)local * REF_STACK);
    g_fiber = (ucontext_t *)malloc((size_t)local * sizeof(ucontext_t));
    g_done = (char *)malloc((size_t)local);
    if (!stacks || !g_fiber || !g_done) { free(stacks); free(g_fiber); free(g_done); return -1; }
    g_args = args;
    g_global = global;
    for (g_base = 0; g_base < global; g_base += local) {
        for (int i = 0; i < local; ++i) {
            getcontext(&g_fiber[i]);
            g_fiber[i].uc_stack.ss_sp = stacks + (size_t)i * REF_STACK;
            g_fiber[i].uc_stack.ss_size = REF_STACK;
            g_fiber[i].uc_link = &g_sched;
            makecontext(&g_fiber[i], fiber_main, 0);
            g_done[i] = 0;
        }
        for (int live = local; live > 0;) {
            for (int i = 0; i < local; ++i) {
                if (g_done[i]) continue;
                g_cur = i;
                swapcontext(&g_sched, &g_fiber[i]);
                if (g_done[i]) --live;
            }
        }
    }
    free(stacks); free(g_fiber); free(g_done);
    return 0;
}
