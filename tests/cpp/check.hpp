// The one check macro and the one closing line of the programs in this directory (tests/cpp_program.py's runner looks for
// the exit status and the line):
//   CHECK(cond)              prints FAILED file:line: cond, counts the failure and goes on
//   CHECK(cond, fmt, ...)    the same, with a printf message behind the condition
//   return check_done();     prints ALL PASSED or FAILED (n); its value is the process's exit status
#pragma once
#include <cstdarg>
#include <cstdio>

inline int g_check_failed = 0;

inline void check_failed(const char *file, int line, const char *cond, const char *fmt, ...)
{
    if (g_check_failed++ >= 20) return;  // a check inside a loop says so twenty times, not a million; the count goes on
    std::printf("FAILED %s:%d: %s", file, line, cond);
    if (*fmt) {
        va_list args;
        va_start(args, fmt);
        std::printf("  ");
        std::vprintf(fmt, args);
        va_end(args);
    }
    std::printf("\n");
}

#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) check_failed(__FILE__, __LINE__, #cond, "" __VA_ARGS__);     \
    } while (0)

inline int check_done()
{
    if (g_check_failed)
        std::printf("FAILED (%d)\n", g_check_failed);
    else
        std::printf("ALL PASSED\n");
    return g_check_failed ? 1 : 0;
}
