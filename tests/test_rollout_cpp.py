"""The trajectory rollouts' host code under sanitizers: tests/cpp/test_rollout.cpp compiles csrc/rollout_host.cpp (with
csrc/visibility_host.cpp, the table's home) and the shared rule csrc/rollout_rule.hpp -- every refusal of the validation,
the reach bound behind the staged window, launch shapes, the key's bit budget, the helpers -- under
-fsanitize=address,undefined into a program of its own, with no HIP header on its include path, and runs the rule against
vectors tests/rollout_ref.py writes: the table, poses step by step and in closed form, pose tests.  The C++ mirror's rollout
part compiles and its host-only helpers run.  Host code only: no GPU needed, and nothing is loaded into Python but the
library for its table."""
import numpy as np

from tests import cpp_program
from tests import navfield_scenes as S
from tests import rollout_ref as R

CELL = 32768


def write_vectors(path, table):
    rng = np.random.default_rng(77)
    out = [str(R.TABLE), " ".join(str(int(v)) for v in table.reshape(-1))]
    # motions: chunk and segment boundaries in every order, both signs, v = 0, +-32767, a w that wraps
    shapes = [(1, 1), (1, 63), (1, 64), (1, 65), (2, 65), (8, 128), (3, 7), (8, 1)]
    out.append(str(len(shapes)))
    for i, (segments, tn) in enumerate(shapes):
        state = (int(rng.integers(-(1 << 29), 1 << 29)), int(rng.integers(-(1 << 29), 1 << 29)), int(rng.integers(0, 65536)))
        cmd = np.stack([rng.integers(-32767, 32768, segments), rng.integers(-32768, 32768, segments)], axis=1)
        cmd[0] = [(0, 900), (32767, -1), (-32767, 30000), (-5, 5)][i % 4]
        p = R.params(segments, tn)
        poses = R.poses(p, state, cmd.tolist(), table)
        out.append(f"{segments} {tn} {state[0]} {state[1]} {state[2]}")
        out.append(" ".join(str(int(v)) for v in cmd.reshape(-1)))
        out.append(" ".join(f"{x} {y} {a}" for x, y, a in poses))
    # pose tests: every code, both unknown rules, footprints that leave the grid on the negative side
    scenes = [(33, 31, 100, -1, 5), (20, 17, 50, 7, 1), (9, 40, 100, 7, 64), (1, 1, 50, -1, 3)]
    out.append(str(len(scenes)))
    for w, h, lethal_min, unknown_cost, f in scenes:
        plane = S.random_plane(rng, w, h, obstacles=0.02, unknown=0.05)
        fp = rng.integers(-300, 301, (f, 2))
        p = R.params(1, 1, lethal_min, unknown_cost)
        out.append(f"{w} {h} {lethal_min} {unknown_cost}")
        out.append(" ".join(str(int(v)) for v in plane.reshape(-1)))
        out.append(str(f))
        out.append(" ".join(str(int(v)) for v in fp.reshape(-1)))
        out.append("200")
        for _ in range(200):
            pose = (int(rng.integers(-2 * CELL, (w + 2) * CELL)), int(rng.integers(-2 * CELL, (h + 2) * CELL)), int(rng.integers(0, 65536)))
            code, cost = R.pose_test(plane, pose, fp.tolist(), table, p)
            out.append(f"{pose[0]} {pose[1]} {pose[2]} {code} {cost}")
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")


def test_rollout_host_and_rule_under_sanitizers(tmp_path, lom):
    vectors = str(tmp_path / "vectors.txt")
    write_vectors(vectors, lom.visibilityTable(R.TABLE))
    exe = cpp_program.build_host(tmp_path, "test_rollout.cpp", ["rollout_host.cpp", "visibility_host.cpp"])
    assert "vectors:" in cpp_program.run(exe, vectors, timeout=300)


def test_cpp_mirror_compiles_and_its_helpers_run(tmp_path):
    """lom::RolloutGrid and the helpers of the C++ mirror compile with plain g++; without an argument the program only runs
    the helpers, which need no device (tests/test_rollout_gpu.py runs the rest)."""
    cpp_program.run(cpp_program.build_with_library(tmp_path, "test_rollout_mirror.cpp"), timeout=120)
