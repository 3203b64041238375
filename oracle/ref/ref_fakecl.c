/*
 * ref_fakecl.c -- stand-in OpenCL runtime for the reference's unmodified host
 * program (TEST INFRASTRUCTURE ONLY).  It offers
 * exactly the entry points that program calls: buffers are host memory, the
 * one kernel is the reference's time_dev compiled as C, and an NDRange is
 * ref_sched.c's ref_launch.  Three platforms are reported so that the `dev`
 * argument may be 0, 1 or 2.  The kernel work-group size reported comes from
 * REF_WG_SIZE (default 8192): every chain up to N = 8191 is one work-group.
 */
#include <stdlib.h>
#include <string.h>
#include <CL/cl.h>

int ref_launch(void *args[19], int global, int local);

static void *g_args[19];
static char g_platforms[3], g_device, g_handle;

static size_t wg_size(void)
{
    const char *e = getenv("REF_WG_SIZE");
    long v = e ? atol(e) : 0;
    return v > 0 ? (size_t)v : 8192;
}

static cl_int put(const void *src, size_t n, size_t size, void *value, size_t *ret)
{
    if (ret) *ret = n;
    if (value && size >= n) memcpy(value, src, n);
    return CL_SUCCESS;
}

cl_int clGetPlatformIDs(cl_uint n, cl_platform_id *ids, cl_uint *count)
{
    if (count) *count = 3;
    for (cl_uint i = 0; ids && i < n && i < 3; ++i) ids[i] = (cl_platform_id)&g_platforms[i];
    return CL_SUCCESS;
}

cl_int clGetDeviceIDs(cl_platform_id p, cl_device_type t, cl_uint n, cl_device_id *ids, cl_uint *count)
{
    (void)p; (void)t;
    if (count) *count = 1;
    if (ids && n >= 1) ids[0] = (cl_device_id)&g_device;
    return CL_SUCCESS;
}

cl_int clGetDeviceInfo(cl_device_id d, cl_device_info what, size_t size, void *value, size_t *ret)
{
    (void)d;
    if (what == CL_DEVICE_MAX_COMPUTE_UNITS) { cl_uint u = 1; return put(&u, sizeof u, size, value, ret); }
    if (what == CL_DEVICE_MAX_WORK_GROUP_SIZE) { size_t s = wg_size(); return put(&s, sizeof s, size, value, ret); }
    return put("serial", 7, size, value, ret);
}

cl_context clCreateContext(const cl_context_properties *p, cl_uint n, const cl_device_id *d,
                           void (*cb)(const char *, const void *, size_t, void *), void *ud, cl_int *err)
{
    (void)p; (void)n; (void)d; (void)cb; (void)ud;
    if (err) *err = CL_SUCCESS;
    return (cl_context)&g_handle;
}

cl_command_queue clCreateCommandQueue(cl_context c, cl_device_id d, cl_command_queue_properties p, cl_int *err)
{
    (void)c; (void)d; (void)p;
    if (err) *err = CL_SUCCESS;
    return (cl_command_queue)&g_handle;
}

cl_mem clCreateBuffer(cl_context c, cl_mem_flags fl, size_t size, void *host, cl_int *err)
{
    (void)c; (void)fl; (void)host;
    if (err) *err = CL_SUCCESS;
    return (cl_mem)calloc(1, size ? size : 1);
}

cl_int clEnqueueWriteBuffer(cl_command_queue q, cl_mem m, cl_bool blocking, size_t off, size_t size,
                            const void *src, cl_uint nw, const cl_event *w, cl_event *ev)
{
    (void)q; (void)blocking; (void)nw; (void)w; (void)ev;
    memcpy((char *)m + off, src, size);
    return CL_SUCCESS;
}

cl_int clEnqueueReadBuffer(cl_command_queue q, cl_mem m, cl_bool blocking, size_t off, size_t size, void *dst,
                           cl_uint nw, const cl_event *w, cl_event *ev)
{
    (void)q; (void)blocking; (void)nw; (void)w; (void)ev;
    memcpy(dst, (const char *)m + off, size);
    return CL_SUCCESS;
}

cl_program clCreateProgramWithSource(cl_context c, cl_uint n, const char **s, const size_t *l, cl_int *err)
{
    (void)c; (void)n; (void)s; (void)l;
    if (err) *err = CL_SUCCESS;
    return (cl_program)&g_handle;
}

cl_int clBuildProgram(cl_program p, cl_uint n, const cl_device_id *d, const char *o,
                      void (*cb)(cl_program, void *), void *ud)
{
    (void)p; (void)n; (void)d; (void)o; (void)cb; (void)ud;
    return CL_SUCCESS;
}

cl_int clGetProgramBuildInfo(cl_program p, cl_device_id d, cl_program_build_info what, size_t size, void *value,
                             size_t *ret)
{
    (void)p; (void)d; (void)what;
    return put("", 1, size, value, ret);
}

cl_kernel clCreateKernel(cl_program p, const char *name, cl_int *err)
{
    (void)p; (void)name;
    if (err) *err = CL_SUCCESS;
    return (cl_kernel)&g_handle;
}

cl_int clSetKernelArg(cl_kernel k, cl_uint idx, size_t size, const void *value)
{
    (void)k;
    if (idx >= 19 || size != sizeof(cl_mem)) return -1;
    g_args[idx] = (void *)*(const cl_mem *)value;
    return CL_SUCCESS;
}

cl_int clGetKernelWorkGroupInfo(cl_kernel k, cl_device_id d, cl_kernel_work_group_info what, size_t size,
                                void *value, size_t *ret)
{
    (void)k; (void)d; (void)what;
    size_t s = wg_size();
    return put(&s, sizeof s, size, value, ret);
}

cl_int clEnqueueNDRangeKernel(cl_command_queue q, cl_kernel k, cl_uint dim, const size_t *off, const size_t *global,
                              const size_t *local, cl_uint nw, const cl_event *w, cl_event *ev)
{
    (void)q; (void)k; (void)dim; (void)off; (void)nw; (void)w; (void)ev;
    return ref_launch(g_args, (int)global[0], (int)local[0]) == 0 ? CL_SUCCESS : -1;
}

cl_int clFinish(cl_command_queue q) { (void)q; return CL_SUCCESS; }
cl_int clFlush(cl_command_queue q) { (void)q; return CL_SUCCESS; }
cl_int clReleaseKernel(cl_kernel k) { (void)k; return CL_SUCCESS; }
cl_int clReleaseProgram(cl_program p) { (void)p; return CL_SUCCESS; }
cl_int clReleaseMemObject(cl_mem m) { free(m); return CL_SUCCESS; }
cl_int clReleaseCommandQueue(cl_command_queue q) { (void)q; return CL_SUCCESS; }
cl_int clReleaseContext(cl_context c) { (void)c; return CL_SUCCESS; }
