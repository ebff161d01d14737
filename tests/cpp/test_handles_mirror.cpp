// The eleven classes of the C++ mirror (include/lidar_odometry_amd.hpp) that own a handle of the C ABI: none can be copied;
// without an argument, where no device is visible, every constructor throws what its family's create returned with the text
// lom_<family>_last_error(NULL) gives (lom::FrontEnd: the literal), a line per class (tests/test_handles_cpp.py).  With
// "device": every class at the smallest size its create takes -- the grids 3 x 2 cells of 0.5 m, whose geometry comes back bit
// for bit with six cells -- clear(), one call that the library refuses with LOM_ERR_ARG before any launch and that must
// throw that code with the handle's own last error (a line per class again), and the destructors.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "lidar_odometry_amd.hpp"

template <typename... T>
constexpr bool none_copyable = (... && (!std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value));
static_assert(none_copyable<lom::FrontEnd, lom::PlaceDatabase, lom::PoseGraph, lom::ScanArchive, lom::OccupancyGrid, lom::ElevationGrid,
                            lom::ClearanceGrid, lom::NavField, lom::RegionGrid, lom::VisibilityGrid, lom::RolloutGrid>,
              "a handle has one owner");

static const lom_occupancy_geometry kGeo{0.5f, -1.f, 2.f, 3, 2};
static const lom_elevation_geometry kElevGeo{0.5f, -1.f, 2.f, 3, 2, 0.25f};
static const lom_place_params kPlace{1, 1, 1.f, 0.f};

// the constructor of T throws (rc, text)
template <typename T, typename... A>
static bool refuses(const char *name, int rc, const std::string &text, A &&...args)
{
    try {
        T made(std::forward<A>(args)...);
    } catch (const lom::Error &e) {
        std::printf("%s %d %s\n", name, e.code, e.what());
        return rc != LOM_OK && e.code == rc && text == e.what();
    }
    std::printf("%s: constructed\n", name);
    return false;
}

// rc: what lom_<family>_create returned for the arguments the constructor passes on
#define REFUSES(T, family, rc, ...)                                   \
    do {                                                              \
        const int rc_ = (rc);                                         \
        const std::string text_ = lom_##family##_last_error(nullptr); \
        if (!refuses<lom::T>(#T, rc_, text_, __VA_ARGS__)) return 1;  \
    } while (0)

static int without_device()
{
    {
        lom_frontend *h = nullptr;
        if (!refuses<lom::FrontEnd>("FrontEnd", lom_frontend_create(0, nullptr, &h), "lom_frontend_create", 0) || h) return 1;
    }
    lom_place_db *db = nullptr;
    REFUSES(PlaceDatabase, place_db, lom_place_db_create(&kPlace, 0, 0, &db), kPlace, (size_t)0, 0);
    lom_graph *graph = nullptr;
    REFUSES(PoseGraph, graph, lom_graph_create(0, 0, 0, &graph), (size_t)0, (size_t)0, 0);
    lom_archive *archive = nullptr;
    REFUSES(ScanArchive, archive, lom_archive_create(0, 0, 0, &archive), (size_t)0, (size_t)0, 0);
    lom_occupancy *occupancy = nullptr;
    REFUSES(OccupancyGrid, occupancy, lom_occupancy_create(&kGeo, 0, &occupancy), kGeo, 0);
    lom_elevation *elevation = nullptr;
    REFUSES(ElevationGrid, elevation, lom_elevation_create(&kElevGeo, 0, &elevation), kElevGeo, 0);
    lom_clearance *clearance = nullptr;
    REFUSES(ClearanceGrid, clearance, lom_clearance_create(&kGeo, 0, &clearance), kGeo, 0);
    lom_navfield *navfield = nullptr;
    REFUSES(NavField, navfield, lom_navfield_create(&kGeo, 0, &navfield), kGeo, 0);
    lom_regions *regions = nullptr;
    REFUSES(RegionGrid, regions, lom_regions_create(&kGeo, 0, &regions), kGeo, 0);
    lom_visibility *visibility = nullptr;
    REFUSES(VisibilityGrid, visibility, lom_visibility_create(&kGeo, 0, &visibility), kGeo, 0);
    lom_rollout *rollout = nullptr;
    REFUSES(RolloutGrid, rollout, lom_rollout_create(&kGeo, 0, &rollout), kGeo, 0);
    if (db || graph || archive || occupancy || elevation || clearance || navfield || regions || visibility || rollout) return 1;
    std::printf("ALL PASSED\n");
    return 0;
}

// `call` throws LOM_ERR_ARG with the text the handle's own last error then reads
template <typename F, typename E>
static bool refused_by_handle(const char *name, F call, E last_error)
{
    try {
        call();
    } catch (const lom::Error &e) {
        std::printf("%s %d %s\n", name, e.code, e.what());
        return e.code == LOM_ERR_ARG && std::strcmp(e.what(), last_error()) == 0;
    }
    return false;
}

// a grid of 3 x 2 cells: the geometry comes back bit for bit, six cells, clear(), an option nobody knows, and out of scope
template <typename T, typename G, auto LastError, typename Count>
static bool grid(const char *name, const G &geo, Count count)
{
    T g(geo);
    const G back = g.geometry();
    if (std::memcmp(&back, &geo, sizeof geo) != 0 || count(g) != 6 || g.device() != 0 || !g.stream()) return false;
    void (T::*wait_event)(void *) = &T::waitEvent;  // every grid has one; none is called here
    if (!wait_event) return false;
    g.clear();
    return refused_by_handle(name, [&] { g.setOption(9999, 0); }, [&] { return LastError(g.handle()); }) && *LastError(g.handle());
}

static bool with_device()
{
    const auto size = [](const auto &g) { return g.size(); };
    {
        lom::FrontEnd fe(0);
        const lom::NeighbourhoodParams no_radius{0.f, 1, 3, 0.1f, 0.f};
        if (!refused_by_handle("FrontEnd", [&] { fe.setClassifier(LOM_CLASSIFIER_NEIGHBOURHOOD, &no_radius); },
                               [&] { return lom_frontend_last_error(fe.handle()); }))
            return false;
    }
    {
        lom::PlaceDatabase db(kPlace);
        db.clear();
        if (db.size() != 0 || db.cells() != 1 || std::memcmp(&db.params(), &kPlace, sizeof kPlace) != 0) return false;
        // no entry with this id
        if (!refused_by_handle("PlaceDatabase", [&] { db.get(0); }, [&] { return lom_place_db_last_error(db.handle()); })) return false;
    }
    {
        lom::PoseGraph graph;
        graph.clear();
        if (graph.nodeCount() != 0 || graph.edgeCount() != 0) return false;
        const lom::GraphPose identity{{0, 0, 0}, {1, 0, 0, 0}};  // an edge that names a node that does not exist
        if (!refused_by_handle("PoseGraph", [&] { graph.addEdge(-1, 0, identity, std::vector<double>(36, 0.0), 0.0); },
                               [&] { return lom_graph_last_error(graph.handle()); }))
            return false;
    }
    {
        lom::ScanArchive archive;
        archive.clear();
        lom::PointCloud<lom::PointNormal> cloud;  // a coordinate that is not finite
        cloud.points.emplace_back(std::nanf(""), 0.f, 0.f);
        if (!refused_by_handle("ScanArchive", [&] { archive.add(cloud); }, [&] { return lom_archive_last_error(archive.handle()); })) return false;
        if (archive.size() != 0 || archive.pointCount() != 0) return false;
    }
    return grid<lom::OccupancyGrid, lom_occupancy_geometry, lom_occupancy_last_error>("OccupancyGrid", kGeo, [](const auto &g) { return g.cells(); }) &&
           grid<lom::ElevationGrid, lom_elevation_geometry, lom_elevation_last_error>("ElevationGrid", kElevGeo, size) &&
           grid<lom::ClearanceGrid, lom_occupancy_geometry, lom_clearance_last_error>("ClearanceGrid", kGeo, size) &&
           grid<lom::NavField, lom_occupancy_geometry, lom_navfield_last_error>("NavField", kGeo, size) &&
           grid<lom::RegionGrid, lom_occupancy_geometry, lom_regions_last_error>("RegionGrid", kGeo, size) &&
           grid<lom::VisibilityGrid, lom_occupancy_geometry, lom_visibility_last_error>("VisibilityGrid", kGeo, size) &&
           grid<lom::RolloutGrid, lom_occupancy_geometry, lom_rollout_last_error>("RolloutGrid", kGeo, size);
}

int main(int argc, char **argv)
{
    if (argc < 2 || std::strcmp(argv[1], "device") != 0) {
        if (lom_device_count() > 0) {
            std::printf("a device is visible: nothing to refuse\n");
            return 0;
        }
        return without_device();
    }
    if (!with_device()) return 2;
    std::printf("ALL PASSED\n");
    return 0;
}
