/*
 * ref_shim.h -- lets a C compiler read the reference's OpenCL C kernel file
 * unchanged (TEST INFRASTRUCTURE ONLY).
 *
 * The kernel file is never copied: ref_kernel.c includes it by the path the
 * build passes in.  What OpenCL C provides and ISO C does not is supplied
 * here, so that every expression of the kernel keeps the meaning an OpenCL
 * compiler gives it:
 *   - <tgmath.h>: sqrt / cos / log / tanh / pow of a float argument are the
 *     float functions, as OpenCL's overloads are;
 *   - pown(float, int), ulong, the address-space qualifiers;
 *   - isinf / isnan return exactly 0 or 1 (glibc's isinf gives -1 for -inf,
 *     and the kernel compares the result with 1);
 *   - the kernel's random() is renamed, libc has one of its own.
 * The work-item functions are ref_sched.c's.
 */
#ifndef REF_SHIM_H
#define REF_SHIM_H
#include <tgmath.h>

typedef unsigned long ulong;

#define __kernel
#define __global
#define __constant const
#define CLK_GLOBAL_MEM_FENCE 2

#define random cl_random

static inline float pown(float x, int n) { return (float)pow((double)x, (double)n); }

#undef isinf
#undef isnan
#define isinf(v) (__builtin_isinf(v) ? 1 : 0)
#define isnan(v) (__builtin_isnan(v) ? 1 : 0)

int get_global_id(int dim);
int get_global_size(int dim);
void barrier(int flags);

#endif
