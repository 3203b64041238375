/* The reference's kernel file as one C translation unit (TEST INFRASTRUCTURE
 * ONLY): build with -DREF_KERNEL='"<reference>/tau_kernel.cl"'. */
#include "ref_shim.h"
#include REF_KERNEL
