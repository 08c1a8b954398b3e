// refusal.hpp — the text of a refused call, for the entry points that live outside bsx_api.hip (live.cpp) and therefore cannot reach a context's fields.
#pragma once

struct bsx_ctx;

namespace bsx {

// Returns BSX_EINVAL and leaves "error: <fn>: <text>" as bsx_last_error(c) and as bsx_last_error(NULL) of the calling thread (c may be NULL: a call refused
// before it knows its context).  Called only for a refused call, before anything is enqueued.
int refuse_call(bsx_ctx* c, const char* fn, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

}  // namespace bsx
