/*
 * CL/cl.h -- the part of the OpenCL 1.2 host API that the reference's host
 * program uses, declared for ref_fakecl.c's stand-in runtime (TEST
 * INFRASTRUCTURE ONLY).  Written from the OpenCL 1.2 specification's function
 * prototypes; the values of the constants matter only inside the stand-in.
 */
#ifndef REF_CL_H
#define REF_CL_H
#include <stddef.h>

typedef int cl_int;
typedef unsigned int cl_uint;
typedef unsigned long cl_ulong;
typedef cl_uint cl_bool;
typedef cl_ulong cl_bitfield;
typedef cl_bitfield cl_device_type;
typedef cl_bitfield cl_mem_flags;
typedef cl_bitfield cl_command_queue_properties;
typedef cl_uint cl_device_info;
typedef cl_uint cl_program_build_info;
typedef cl_uint cl_kernel_work_group_info;
typedef long cl_context_properties;

typedef struct ref_cl_platform *cl_platform_id;
typedef struct ref_cl_device *cl_device_id;
typedef struct ref_cl_context *cl_context;
typedef struct ref_cl_queue *cl_command_queue;
typedef struct ref_cl_mem *cl_mem;
typedef struct ref_cl_program *cl_program;
typedef struct ref_cl_kernel *cl_kernel;
typedef struct ref_cl_event *cl_event;

#define CL_SUCCESS 0
#define CL_BUILD_PROGRAM_FAILURE (-11)
#define CL_TRUE 1
#define CL_FALSE 0
#define CL_DEVICE_TYPE_DEFAULT 1
#define CL_MEM_READ_WRITE 1
#define CL_MEM_WRITE_ONLY 2
#define CL_MEM_READ_ONLY 4
#define CL_DEVICE_MAX_COMPUTE_UNITS 0x1002
#define CL_DEVICE_MAX_WORK_GROUP_SIZE 0x1004
#define CL_DEVICE_NAME 0x102B
#define CL_DRIVER_VERSION 0x102D
#define CL_DEVICE_VERSION 0x102F
#define CL_DEVICE_OPENCL_C_VERSION 0x103D
#define CL_PROGRAM_BUILD_LOG 0x1183
#define CL_KERNEL_WORK_GROUP_SIZE 0x11B0

cl_int clGetPlatformIDs(cl_uint, cl_platform_id *, cl_uint *);
cl_int clGetDeviceIDs(cl_platform_id, cl_device_type, cl_uint, cl_device_id *, cl_uint *);
cl_int clGetDeviceInfo(cl_device_id, cl_device_info, size_t, void *, size_t *);
cl_context clCreateContext(const cl_context_properties *, cl_uint, const cl_device_id *,
                           void (*)(const char *, const void *, size_t, void *), void *, cl_int *);
cl_command_queue clCreateCommandQueue(cl_context, cl_device_id, cl_command_queue_properties, cl_int *);
cl_mem clCreateBuffer(cl_context, cl_mem_flags, size_t, void *, cl_int *);
cl_int clEnqueueWriteBuffer(cl_command_queue, cl_mem, cl_bool, size_t, size_t, const void *, cl_uint,
                            const cl_event *, cl_event *);
cl_int clEnqueueReadBuffer(cl_command_queue, cl_mem, cl_bool, size_t, size_t, void *, cl_uint, const cl_event *,
                           cl_event *);
cl_program clCreateProgramWithSource(cl_context, cl_uint, const char **, const size_t *, cl_int *);
cl_int clBuildProgram(cl_program, cl_uint, const cl_device_id *, const char *, void (*)(cl_program, void *),
                      void *);
cl_int clGetProgramBuildInfo(cl_program, cl_device_id, cl_program_build_info, size_t, void *, size_t *);
cl_kernel clCreateKernel(cl_program, const char *, cl_int *);
cl_int clSetKernelArg(cl_kernel, cl_uint, size_t, const void *);
cl_int clGetKernelWorkGroupInfo(cl_kernel, cl_device_id, cl_kernel_work_group_info, size_t, void *, size_t *);
cl_int clEnqueueNDRangeKernel(cl_command_queue, cl_kernel, cl_uint, const size_t *, const size_t *,
                              const size_t *, cl_uint, const cl_event *, cl_event *);
cl_int clFinish(cl_command_queue);
cl_int clFlush(cl_command_queue);
cl_int clReleaseKernel(cl_kernel);
cl_int clReleaseProgram(cl_program);
cl_int clReleaseMemObject(cl_mem);
cl_int clReleaseCommandQueue(cl_command_queue);
cl_int clReleaseContext(cl_context);

#endif
