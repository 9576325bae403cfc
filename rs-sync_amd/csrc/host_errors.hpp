// host_errors.hpp -- the library's error convention (core_support/panic.cpp:7-15), shared by the host files of
// librssync_core.so (sync_problem.cpp defines it, track_api.cpp uses it).  Internal: hidden visibility, not part of any
// public header.
#pragma once

#include <stdexcept>
#include <string>

namespace rssync_host __attribute__((visibility("hidden"))) {

struct PanicError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

extern int g_panic_mode; // 0 = reference behaviour, 1 = throw (caught by the C-ABI)
extern thread_local std::string g_last_error;

// mode 0: panic.txt + the reason on stderr + exit(1); mode 1: throw PanicError
[[noreturn]] void panic(const std::string& reason);

// a C-ABI body: 0 = ok, 1 = panic (message in g_last_error), 2 = other exception
template <typename F>
int guarded(F&& f) {
    try {
        f();
        return 0;
    } catch (const PanicError& e) {
        g_last_error = e.what();
        return 1;
    } catch (const std::exception& e) {
        g_last_error = std::string("exception: ") + e.what();
        return 2;
    }
}

} // namespace rssync_host
