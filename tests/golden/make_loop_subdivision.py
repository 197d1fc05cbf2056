"""Writes tests/golden/loop_subdivision.npz: what the REFERENCE's ``loop_subdivision`` (deodr/triangulated_mesh.py:499-562) returns.

Run on the build machine only (needs the reference tree):  python tests/golden/make_loop_subdivision.py [path of the reference]

The reference's ``deodr/triangulated_mesh.py`` and ``deodr/tools.py`` are loaded from its tree as they are, under a package stub, with a stub for
the ``trimesh.base.Trimesh`` type name (only an annotation there; trimesh is not installed) -- as tests/golden/make_golden.py does.  Nothing of the
reference's source is written into this repository; the fixture is data:

  octa_vertices / octa_faces / octa_colors     the octahedron with random colours (the input)
  octa{1,2}_vertices / _faces / _colors        the reference's result at 1 and 2 levels
  hand1_vertices / hand1_faces                 tests/golden/hand_mesh.npz at 1 level
  hand2_vertices / hand2_faces_sha256          ... at 2 levels: the vertices and the SHA-256 of the faces as contiguous int64 bytes
"""

import hashlib
import importlib.util
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))


def load_reference(root):
    trimesh, base = types.ModuleType("trimesh"), types.ModuleType("trimesh.base")
    base.Trimesh = type("Trimesh", (), {})
    trimesh.base = base
    sys.modules.update({"trimesh": trimesh, "trimesh.base": base})
    package = types.ModuleType("deodr")
    package.__path__ = [os.path.join(root, "deodr")]
    sys.modules["deodr"] = package
    for name in ("tools", "triangulated_mesh"):
        spec = importlib.util.spec_from_file_location("deodr." + name, os.path.join(root, "deodr", name + ".py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules["deodr." + name] = module
        spec.loader.exec_module(module)
    return sys.modules["deodr.triangulated_mesh"]


def octahedron():
    vertices = np.array([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    faces = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    return vertices, faces, np.random.RandomState(0).rand(6, 3)


def main():
    tm = load_reference(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DEODR_REFERENCE", "/root/reference"))
    out = {}
    vertices, faces, colors = octahedron()
    out.update(octa_vertices=vertices, octa_faces=faces.astype(np.int32), octa_colors=colors)
    for level in (1, 2):
        m = tm.loop_subdivision(tm.ColoredTriMesh(faces, vertices=vertices, colors=colors), level)
        out.update({f"octa{level}_vertices": m.vertices, f"octa{level}_faces": m.faces.astype(np.int32), f"octa{level}_colors": m.vertices_colors})
    hand = np.load(os.path.join(OUT, "hand_mesh.npz"))
    mesh = tm.ColoredTriMesh(hand["faces"].astype(np.int64), vertices=hand["vertices"], nb_colors=0)
    m1, m2 = tm.loop_subdivision(mesh, 1), tm.loop_subdivision(mesh, 2)
    assert m1.vertices.shape == (2098, 3) and m1.faces.shape == (4192, 3) and m2.vertices.shape == (8386, 3) and m2.faces.shape == (16768, 3)
    out.update(hand1_vertices=m1.vertices, hand1_faces=m1.faces.astype(np.int32), hand2_vertices=m2.vertices,
               hand2_faces_sha256=np.array(hashlib.sha256(np.ascontiguousarray(m2.faces.astype(np.int64)).tobytes()).hexdigest()))  # fmt: skip
    path = os.path.join(OUT, "loop_subdivision.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(OUT, "rgb_hand_fit.npz"))


if __name__ == "__main__":
    main()
