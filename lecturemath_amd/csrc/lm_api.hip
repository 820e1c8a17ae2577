// lm_api.hip -- the translation unit of the library: it includes every other file of this directory, so that each launch sees its
// kernel's definition, and holds what all of them share -- the error string, lm_blocks, lm_alloc and the three exports that describe the build.
#include "lm_common.h"
#include "lm_stream.h"

#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include "../../include/lecturemath_amd.h"

// the message behind lm_last_error(), per thread
static thread_local char g_err[512] = "";

void lm_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static inline unsigned lm_blocks(long long work_items, int block, int max_blocks = 8192)
{
    long long b = (work_items + block - 1) / block;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return (unsigned)b;
}

template <class T> static int lm_alloc(T** p, size_t count)
{
    LM_HIP(hipMalloc((void**)p, count * sizeof(T) + 64));
    return LM_OK;
}

extern "C" const char* lm_last_error(void) { return g_err; }
extern "C" int lm_abi_version(void) { return 1; }
extern "C" int lm_is_device_build(void) { return LM_HIP_EMULATED ? 0 : 1; }

// Order constraints: every file may use what stands above this block.  The entry points follow the kernels they launch: lm_ctx.hip after
// lm_cc_kernels.hip and lm_fcn_bytes.hip; lm_stream.hip after lm_ctx.hip, lm_match_kernels.hip and lm_match_batch.hip; lm_handoff.hip after
// lm_stream.hip; lm_legacy.hip after lm_ctx.hip; lm_keyframes.hip after lm_group.hip; lm_ccmatch.hip after lm_keyframes.hip; lm_kfcc.hip
// after lm_ctx.hip and lm_ccmatch.hip; lm_history.hip after lm_keyframes.hip.  Kernels reach the code object in the order of this list.
#include "lm_cc_kernels.hip"
#include "lm_fcn_bytes.hip"
#include "lm_match_kernels.hip"
#include "lm_match_batch.hip"
#include "lm_group.hip"
#include "lm_fcn.hip"
#include "lm_fcn2.hip"
#include "lm_ctx.hip"
#include "lm_stream.hip"
#include "lm_handoff.hip"
#include "lm_legacy.hip"
#include "lm_resize.hip"
#include "lm_png.hip"
#include "lm_segment.hip"
#include "lm_keyframes.hip"
#include "lm_align.hip"
#include "lm_ccmatch.hip"
#include "lm_kfcc.hip"
#include "lm_history.hip"
