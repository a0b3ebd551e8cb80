// devbuf_failure.hip -- stand-alone host program (tests/test_devbuf_cpu.py builds it with the host side under
// AddressSanitizer and UndefinedBehaviorSanitizer): the failure paths of jdsp::DevBuf on a machine without a device,
// where every hipMalloc fails and nothing has to be injected.  Exit status 0: every check held; 77: a device is
// present, so nothing would fail and nothing was checked.
#include "../jeicyboodsp_amd/csrc/jdsp_internal.h"

#include <utility>

static int g_failed = 0;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            g_failed++;                                                   \
        }                                                                 \
    } while (0)

template <class T> static bool empty(const jdsp::DevBuf<T> &b) { return b.get() == nullptr && b.count() == 0; }

int main()
{
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0) return 77;

    const float host[4] = {1.f, 2.f, 3.f, 4.f};
    {
        jdsp::DevBuf<float> fresh;                   // never used: destroyed empty
        CHECK(empty(fresh));
    }
    {
        jdsp::DevBuf<float> a;
        CHECK(a.alloc(4) != hipSuccess);
        CHECK(empty(a));
        CHECK(a.upload(host, 4) != hipSuccess);
        CHECK(empty(a));
        CHECK(a.grow(4) != hipSuccess);
        CHECK(empty(a));
        CHECK(a.grow(8) != hipSuccess);              // again, on a buffer that has already failed
        CHECK(empty(a));
        CHECK(a.grow(0) == hipSuccess);              // nothing asked for beyond what it holds: not even an attempt
        CHECK(empty(a));
        a.reset();
        a.reset();
        CHECK(empty(a));

        jdsp::DevBuf<float> b(std::move(a));         // moved from a failed buffer
        CHECK(empty(a) && empty(b));
        jdsp::DevBuf<float> c;
        c = std::move(b);
        CHECK(empty(b) && empty(c));
        c = std::move(c);                            // self-assignment frees nothing
        CHECK(empty(c));
        CHECK(b.grow(2) != hipSuccess);              // a moved-from buffer is an ordinary empty one
        CHECK(empty(b));
    }                                                // failed, moved-from and empty buffers are destroyed here

    // the two owners built on it: all or nothing, and clean to destroy after a failure
    {
        jdsp::RunPlanWs ws;
        CHECK(ws.reserve(70) != hipSuccess);
        CHECK(ws.cap_blocks == 0);
        CHECK(empty(ws.flags) && empty(ws.events) && empty(ws.ev_n) && empty(ws.ver_base) && empty(ws.snap_mask));
        jdsp::RunPlanWs other = std::move(ws);
        CHECK(other.cap_blocks == 0 && empty(other.flags));
    }
    if (g_failed) return 1;
    puts("DevBuf failure paths: ok");
    return 0;
}
