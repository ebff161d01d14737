// The handle core of csrc/device_handle.hpp as a program of its own (tests/test_device_handle_cpp.py), compiled by plain
// g++ under -fsanitize=address,undefined: the size rule of the grow-only buffers, move / swap / release of EMPTY
// DeviceBuf and PinnedBuf (the destructors of empty buffers free nothing), and the error texts of fail / create_fail.
// No HIP call that needs a device is made: the only one reached is hipGetErrorString.
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>
#include <utility>

#include "check.hpp"
#include "device_handle.hpp"

using namespace lom;

struct Family : DeviceHandle {  // as lom_map and the others derive
    int more = 7;
};

static void test_grown_bytes()
{
    // nothing asked for, or enough there: the size stays
    CHECK(grown_bytes(0, 0) == 0);
    CHECK(grown_bytes(256, 0) == 256);
    CHECK(grown_bytes(256, 256) == 256);
    CHECK(grown_bytes(1000, 999) == 1000);  // (not rounded: nothing is allocated)
    // the first block: the request rounded up to 256
    CHECK(grown_bytes(0, 1) == 256);
    CHECK(grown_bytes(0, 255) == 256);
    CHECK(grown_bytes(0, 256) == 256);
    CHECK(grown_bytes(0, 257) == 512);
    // growth: at least 1.5 times the old block
    CHECK(grown_bytes(256, 257) == 512);     // 384 -> 512
    CHECK(grown_bytes(1024, 1025) == 1536);  // exactly 1.5 x, already a multiple of 256
    CHECK(grown_bytes(1000, 1001) == 1536);  // 1500 -> 1536
    CHECK(grown_bytes(1024, 4000) == 4096);  // the request is the larger
    CHECK(grown_bytes(4096, 6144) == 6144);
    CHECK(grown_bytes(4096, 6145) == 6400);
    // every result is a multiple of 256 and covers both the request and the step
    for (size_t have : {size_t(0), size_t(256), size_t(768), size_t(1) << 20, (size_t(1) << 32) + 256})
        for (size_t more : {size_t(1), size_t(100), size_t(255), size_t(256), size_t(100000)}) {
            const size_t got = grown_bytes(have, have + more);
            CHECK(got % 256 == 0 && got >= have + more && got >= have + have / 2 && got < have + have / 2 + more + 256);
        }
    // near SIZE_MAX / 2: 1.5 x still fits, nothing wraps
    const size_t half = SIZE_MAX / 2;
    CHECK(grown_bytes(half, half + 1) >= half + half / 2 && grown_bytes(half, half + 1) % 256 == 0);
    CHECK(grown_bytes(half - 1000, half) >= half);
    CHECK(grown_bytes(0, half) == ((half + 255) & ~size_t(255)));
    // beyond: the result saturates instead of wrapping to something small (the allocation then fails as it should)
    CHECK(grown_bytes(half + half / 2, SIZE_MAX - 1000) >= SIZE_MAX - 1000);
    CHECK(grown_bytes(SIZE_MAX - 4096, SIZE_MAX - 100) >= SIZE_MAX - 100);
    CHECK(grown_bytes(SIZE_MAX - 4096, SIZE_MAX) == SIZE_MAX);
    CHECK(grown_bytes(0, SIZE_MAX) == SIZE_MAX);
}

template <class B>
static bool empty(const B &b);
template <>
bool empty(const DeviceBuf &b) { return b.p == nullptr && b.bytes == 0 && b.as<float>() == nullptr; }
template <>
bool empty(const PinnedBuf &b) { return b.h == nullptr && b.d == nullptr && b.bytes == 0 && b.as<double>() == nullptr; }

template <class B>
static void test_empty_buffers()
{
    static_assert(!std::is_copy_constructible<B>::value && !std::is_copy_assignable<B>::value, "one owner");
    static_assert(std::is_nothrow_move_constructible<B>::value && std::is_nothrow_move_assignable<B>::value, "moves");
    B a, b;
    CHECK(empty(a) && empty(b));
    B c(std::move(a));  // move construction
    CHECK(empty(a) && empty(c));
    b = std::move(c);  // move assignment
    CHECK(empty(b) && empty(c));
    b = std::move(b);  // onto itself
    CHECK(empty(b));
    using std::swap;
    swap(a, b);  // as graph.hip swaps its pose buffers
    a.swap(a);
    CHECK(empty(a) && empty(b));
    release(a);  // "free now" of nothing
    release(a);
    CHECK(empty(a));
    B arr[3];  // as lom_map::scr[], lom_graph::buf[]
    std::swap(arr[0], arr[2]);
    CHECK(empty(arr[0]) && empty(arr[2]));
}  // the destructors of empty buffers run here

static void test_errors()
{
    Family h;
    std::string slot = "create text";
    CHECK(h.error.empty());
    // fail: the handle's text, the code handed through, the create slot left alone
    CHECK(fail(&h, LOM_ERR_ARG, "bad argument") == LOM_ERR_ARG);
    CHECK(h.error == "bad argument" && slot == "create text");
    CHECK(fail(&h, LOM_ERR_OOM, "hipMalloc", hipErrorOutOfMemory) == LOM_ERR_OOM);
    CHECK(h.error == std::string("hipMalloc: ") + hipGetErrorString(hipErrorOutOfMemory));
    CHECK(h.error.size() > std::string("hipMalloc: ").size() && slot == "create text");
    CHECK(fail(&h, LOM_ERR_HIP, nullptr) == LOM_ERR_HIP && h.error.empty());  // no text is an empty text
    // create_fail: the slot's text, the handle left alone
    fail(&h, LOM_ERR_STATE, "handle text");
    CHECK(create_fail(slot, LOM_ERR_NO_DEVICE, "no device") == LOM_ERR_NO_DEVICE);
    CHECK(slot == "no device" && h.error == "handle text");
    CHECK(create_fail(slot, LOM_ERR_HIP, "setup", hipErrorInvalidValue) == LOM_ERR_HIP);
    CHECK(slot == std::string("setup: ") + hipGetErrorString(hipErrorInvalidValue) && h.error == "handle text");
    // two families, two slots
    std::string other = "other family";
    create_fail(slot, LOM_ERR_ARG, "mine");
    CHECK(other == "other family" && slot == "mine");
    // LOM_HIP on a derived handle: returns LOM_ERR_HIP with the expression's text, or falls through
    auto run = [](Family *f, hipError_t e) -> int {
        LOM_HIP(f, e);
        return LOM_OK;
    };
    h.error = "kept";
    CHECK(run(&h, hipSuccess) == LOM_OK && h.error == "kept");
    CHECK(run(&h, hipErrorInvalidValue) == LOM_ERR_HIP);
    CHECK(h.error == std::string("e: ") + hipGetErrorString(hipErrorInvalidValue) && h.more == 7);
}

int main()
{
    test_grown_bytes();
    test_empty_buffers<DeviceBuf>();
    test_empty_buffers<PinnedBuf>();
    test_errors();
    return check_done();
}
