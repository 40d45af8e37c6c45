// gsm_host.h — host helpers of the extern "C" boundary that both of its
// translation units use (gsm_abi.hip: the env handle; gsm_ops.hip: the stateless
// entry points of the training chain).
#pragma once
#include <stdio.h>

#include <initializer_list>
#include <string>

#include "gsm.h"
#include "gsm_internal.h"

#pragma GCC visibility push(hidden)   // the library's own: nothing here is exported

// Records msg as the handle's (h != nullptr) and the thread's last error, what
// gsm_last_error reads, and returns code. Defined in gsm_abi.hip beside the
// handle and the one thread-local string.
int fail(gsm_handle *h, int code, const std::string &msg);

inline int hip_fail(gsm_handle *h, hipError_t e, const char *where) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: hipError %d (%s)", where, (int)e, hipGetErrorString(e));
    return fail(h, GSM_EHIP, buf);
}

// the tail of an entry point that launched: `what` names the step in the error
inline int launched(hipError_t e, const char *what) { return e == hipSuccess ? GSM_OK : hip_fail(nullptr, e, what); }

// argument checks that several entry points share, each with its one message
inline int heads_shape(int32_t heads, int32_t channels) {
    if (heads < 1 || channels < 1 || (channels & (channels - 1)) || heads * channels > 64)
        return fail(nullptr, GSM_EINVAL, "need channels a power of two and heads*channels <= 64");
    return GSM_OK;
}
inline int nodes_range(int64_t n_nodes) {
    return n_nodes < 0 || n_nodes >= ((int64_t)1 << 40) ? fail(nullptr, GSM_EINVAL, "bad n_nodes") : GSM_OK;
}
inline int edges_range(int64_t n_edges) {
    return n_edges < 0 || n_edges >= ((int64_t)1 << 31) ? fail(nullptr, GSM_EINVAL, "bad n_edges") : GSM_OK;
}

// zero bytes at each (pointer, bytes) in order until the first error; a nullptr is skipped
struct Zeroed {
    void *ptr;
    size_t bytes;
};
inline hipError_t zero_all(std::initializer_list<Zeroed> list, hipStream_t s) {
    for (const Zeroed &z : list) {
        if (!z.ptr) continue;
        const hipError_t e = hipMemsetAsync(z.ptr, 0, z.bytes, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

#pragma GCC visibility pop
