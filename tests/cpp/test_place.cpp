// lom::PlaceDatabase of the header-only mirror (include/lidar_odometry_amd.hpp) against the C functions: shiftYaw and
// the refusals, which come before any device work -- host code only, no device is touched.  Built and run by
// tests/test_place_cpp.py.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <limits>
#include <vector>

#include "check.hpp"
#include "lidar_odometry_amd.hpp"

using namespace lom;

static_assert(LOM_ABI_VERSION == 2, "ABI version");
static_assert(sizeof(lom_place_params) == 16 && offsetof(lom_place_params, max_range) == 8, "lom_place_params");
static_assert(sizeof(lom_place_match) == 16 && offsetof(lom_place_match, distance) == 8 && offsetof(lom_place_match, shift) == 12,
              "lom_place_match: the layout the Python binding states");

static bool create_refused(const PlaceParams &p)
{
    lom_place_db *h = nullptr;
    CHECK(lom_place_db_create(&p, 0, 4, &h) == LOM_ERR_ARG && h == nullptr);
    CHECK(std::isnan(lom_place_shift_yaw(&p, 1)));
    bool yaw_thrown = false, create_thrown = false;
    try {
        PlaceDatabase::shiftYaw(p, 1);
    } catch (const Error &e) {
        yaw_thrown = e.code == LOM_ERR_ARG;
    }
    try {
        PlaceDatabase db(p);
    } catch (const Error &e) {
        create_thrown = e.code == LOM_ERR_ARG;
    }
    return yaw_thrown && create_thrown;
}

int main()
{
    const double two_pi = 6.283185307179586476925286766559;
    const PlaceParams good{20, 60, 80.f, -1.5f};
    for (uint32_t shift : {0u, 1u, 7u, 53u, 59u, 60u, 61u}) {
        const double want = (double)((60u - shift % 60u) % 60u) * two_pi / 60.0;
        CHECK(lom_place_shift_yaw(&good, shift) == want);
        CHECK(PlaceDatabase::shiftYaw(good, shift) == want);
    }
    CHECK(PlaceDatabase::shiftYaw(good, 53) == 7.0 * two_pi / 60.0);
    const PlaceParams one{1, 1, 1.f, 0.f}, full{64, 64, 5.f, 2.f};
    CHECK(PlaceDatabase::shiftYaw(one, 0) == 0.0 && PlaceDatabase::shiftYaw(full, 63) == two_pi / 64.0);

    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const PlaceParams bad[] = {{0, 60, 80.f, 0.f},  {65, 60, 80.f, 0.f}, {20, 0, 80.f, 0.f},  {20, 65, 80.f, 0.f},
                               {20, 60, nan, 0.f},  {20, 60, inf, 0.f},  {20, 60, 0.f, 0.f},  {20, 60, -1.f, 0.f},
                               {20, 60, 80.f, nan}, {20, 60, 80.f, inf}};
    for (const PlaceParams &p : bad) CHECK(create_refused(p));

    // NULL handles: refused by the C functions before any device work.  (No handle can be made without a device, so the
    // bad k and ids below check the NULL refusal only; on a live database: tests/test_place_gpu.py.)
    std::vector<float> desc(20 * 60, 0.f), xyz(12, 0.f);
    lom_place_match out[64];
    lom_place_db *h = nullptr;
    CHECK(lom_place_db_create(nullptr, 0, 0, &h) == LOM_ERR_ARG);
    CHECK(lom_place_db_create(&good, 0, 0, nullptr) == LOM_ERR_ARG);
    CHECK(lom_place_db_size(nullptr) == LOM_ERR_ARG && lom_place_db_clear(nullptr) == LOM_ERR_ARG);
    CHECK(lom_place_describe(nullptr, xyz.data(), 4, 12, desc.data()) == LOM_ERR_ARG);
    CHECK(lom_place_db_add(nullptr, desc.data()) == LOM_ERR_ARG);
    CHECK(lom_place_db_add_cloud(nullptr, xyz.data(), 4, 12) == LOM_ERR_ARG);
    CHECK(lom_place_db_get(nullptr, 0, desc.data()) == LOM_ERR_ARG);
    CHECK(lom_place_db_query(nullptr, desc.data(), 1, 0, 0, 0, out, nullptr) == LOM_ERR_ARG);
    CHECK(lom_place_db_query(nullptr, desc.data(), 1, 0, 0, 65, out, nullptr) == LOM_ERR_ARG);
    CHECK(lom_place_db_query(nullptr, desc.data(), 1, 2, 1, 1, out, nullptr) == LOM_ERR_ARG);
    CHECK(lom_odometry_place_descriptor(nullptr, nullptr, 0, desc.data(), nullptr) == LOM_ERR_ARG);
    CHECK(lom_place_db_wait_event(nullptr, nullptr) == LOM_ERR_ARG && lom_place_db_device(nullptr) == LOM_ERR_ARG);
    CHECK(lom_place_db_stream(nullptr) == nullptr && lom_frontend_deskewed(nullptr, nullptr, nullptr) == LOM_ERR_ARG);
    lom_place_db_destroy(nullptr);
    // (the members that need a database -- describe, add, addCloud, get, query, LidarOdometry::placeDescriptor -- compile)
    std::vector<float> (PlaceDatabase::*describe_xyz)(const PointCloud<PointXYZ> &) const = &PlaceDatabase::describe<PointXYZ>;
    int64_t (PlaceDatabase::*add_irt)(const PointCloud<lom_point_xyzirt> &) = &PlaceDatabase::addCloud<lom_point_xyzirt>;
    std::vector<float> (LidarOdometry::*place)(PlaceDatabase &, int64_t *) const = &LidarOdometry::placeDescriptor;
    CHECK(describe_xyz != nullptr && add_irt != nullptr && place != nullptr && &PlaceDatabase::query != nullptr);
    return check_done();
}
