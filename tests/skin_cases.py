"""Test helper (no tests here): seeded generators of small .gltf files with skins and morph targets — the shapes at which the device skinning pass (pt_animate_skinned, k_skin)
can still go wrong — for tests/test_skin_palette.py and tests/test_gpu_device_skinning.py, and, at other sizes, for tools/skinning_ab.py.

  A  the two-joint bar: one mesh of two primitives (float weights, normalised-byte weights) with NORMAL and TANGENT under a translated mesh node with NON-UNIFORM scale; a
     static mesh shares the file
  B  morph targets and a skin on the same primitive: two targets with POSITION, NORMAL and TANGENT displacements, a `weights` animation channel
  C  a strip of 1 061 vertices (a prime: a multiple of neither 64 nor 256) on 70 joints (more than a wave has lanes); every vertex uses 4 joints with random weights
  D  edge records inside one skinned primitive: a vertex with all four weights 0, a joint index beyond the palette, a joint whose animated scale is 0 on one axis at t = 1
     (det == 0), a vertex whose posed normal sums to zero length
  E  two deformed ranges separated by a static mesh, a static mesh before the first and another after the last: the static vertices are the sentinels

Every case returns a dict: path, times (key times and points between them), sentinels (a bool mask over the vertex stream: vertices no pose may touch), light / camera
(a point light's position and scenes.bridge_camera's arguments under which the meshes are in view)."""
import base64, json, math
import numpy as np

F32, U8, U16, U32 = 5126, 5121, 5123, 5125
CASES = ("A", "B", "C", "D", "E")


def quat(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a); s = math.sin(angle / 2)
    return [float(a[0] * s), float(a[1] * s), float(a[2] * s), math.cos(angle / 2)]


class Writer:
    """accumulates accessors over one buffer; write() embeds it as base64, or puts it next to the file (external=True: large files)"""
    def __init__(self):
        self.blob = bytearray(); self.views = []; self.acc = []

    def add(self, arr, typ, normalized=False, bounds=False):
        arr = np.ascontiguousarray(arr); ct = {np.dtype(np.float32): F32, np.dtype(np.uint8): U8, np.dtype(np.uint16): U16, np.dtype(np.uint32): U32}[arr.dtype]
        self.blob += b"\0" * ((-len(self.blob)) % 4); self.views.append({"buffer": 0, "byteOffset": len(self.blob), "byteLength": arr.nbytes}); self.blob += arr.tobytes()
        a = {"bufferView": len(self.views) - 1, "componentType": ct, "count": int(arr.shape[0]), "type": typ}
        if normalized: a["normalized"] = True
        if bounds: a["min"] = arr.min(0).tolist(); a["max"] = arr.max(0).tolist()
        self.acc.append(a); return len(self.acc) - 1

    def write(self, path, doc, external=False):
        doc = dict(doc); doc["asset"] = {"version": "2.0"}; doc["accessors"] = self.acc; doc["bufferViews"] = self.views
        if external:
            binp = path.with_suffix(".bin"); binp.write_bytes(bytes(self.blob)); doc["buffers"] = [{"byteLength": len(self.blob), "uri": binp.name}]
        else:
            doc["buffers"] = [{"byteLength": len(self.blob), "uri": "data:application/octet-stream;base64," + base64.b64encode(bytes(self.blob)).decode()}]
        path.write_text(json.dumps(doc)); return path


def strip(rng, n, length=2.0, width=0.3):
    """n vertices zig-zagging up +Y (n - 2 triangles), random unit normals and tangents (handedness +-1): positions, normals, tangents float32, indices"""
    i = np.arange(n)
    P = np.stack([np.where(i % 2, 0.5 * width, -0.5 * width), np.linspace(0.0, length, n), rng.uniform(-0.05, 0.05, n)], 1).astype(np.float32)
    N = rng.normal(size=(n, 3)); N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)
    T = rng.normal(size=(n, 3)); T = T / np.linalg.norm(T, axis=1, keepdims=True); T = np.concatenate([T, rng.choice([-1.0, 1.0], (n, 1))], 1).astype(np.float32)
    I = np.stack([i[:-2], i[1:-1], i[2:]], 1).reshape(-1).astype(np.uint16 if n < 65536 else np.uint32)
    return P, N, T, I


def primitive(w, P, N, T, I, J=None, W=None, byte_weights=False, targets=None):
    at = {"POSITION": w.add(P, "VEC3", bounds=True), "NORMAL": w.add(N, "VEC3"), "TANGENT": w.add(T, "VEC4")}
    if J is not None:
        at["JOINTS_0"] = w.add(np.asarray(J, np.uint8 if np.max(J) < 256 else np.uint16), "VEC4")
        at["WEIGHTS_0"] = w.add(np.round(np.asarray(W) * 255).astype(np.uint8), "VEC4", normalized=True) if byte_weights else w.add(np.asarray(W, np.float32), "VEC4")
    pr = {"attributes": at, "indices": w.add(I, "SCALAR")}
    if targets: pr["targets"] = [{k: w.add(np.asarray(v, np.float32), "VEC3") for k, v in t.items()} for t in targets]
    return pr


def sampler(w, anim, times, values, typ, node, path, interpolation="LINEAR"):
    anim["samplers"].append({"input": w.add(np.asarray(times, np.float32), "SCALAR"), "output": w.add(np.asarray(values, np.float32), typ), "interpolation": interpolation})
    anim["channels"].append({"sampler": len(anim["samplers"]) - 1, "target": {"node": node, "path": path}})


def ibm_translations(w, ys):
    """inverse bind matrices of joints whose bind-pose worlds are translations by (0, y, 0): MAT4 accessor (column major)"""
    M = np.tile(np.eye(4, dtype=np.float32), (len(ys), 1, 1)); M[:, 3, 1] = -np.asarray(ys, np.float32)      # row 3 of the transposed (= column 3) holds the translation
    return w.add(M.reshape(-1, 16), "MAT4")


VIEW = dict(light=(0.5, 1.5, -3.0), camera=dict(pos=(0.5, 1.0, -6.0), direction=(0.0, 0.0, 1.0), up=(0, 1, 0), fov_y=math.radians(50.0), near_z=0.01, far_z=100.0, focal_distance=1.0))
TIMES = (0.0, 0.35, 1.0, 1.6, 2.0)


def blend_weights(P, joints=(0, 1)):
    w1 = np.clip((P[:, 1] - 0.5) / 1.0, 0, 1); W = np.zeros((len(P), 4), np.float32); W[:, 0] = 1 - w1; W[:, 1] = w1
    J = np.zeros((len(P), 4), np.uint8); J[:, 0] = joints[0]; J[:, 1] = joints[1]; return J, W


def case_a(tmp_path, seed=1):
    rng = np.random.default_rng(seed); w = Writer(); P, N, T, I = strip(rng, 10); J, W = blend_weights(P)
    Ps, Ns, Ts, Is = strip(rng, 7)
    anim = {"samplers": [], "channels": []}
    meshes = [{"primitives": [primitive(w, P, N, T, I, J, W), primitive(w, P, N, T, I, J, W, byte_weights=True)]}, {"primitives": [primitive(w, Ps, Ns, Ts, Is)]}]
    nodes = [{"name": "bar", "mesh": 0, "skin": 0, "translation": [0.5, 0.2, 0.0], "scale": [2.0, 1.5, 0.5]}, {"name": "root", "children": [2]}, {"name": "j0", "children": [3]},
             {"name": "j1", "translation": [0.0, 1.0, 0.0]}, {"name": "static", "mesh": 1, "translation": [-1.0, 0.0, 0.0]}]
    sampler(w, anim, [0.0, 1.0, 2.0], [quat((0, 0, 1), 0.0), quat((0, 0, 1), math.pi / 2), quat((1, 0, 1), 0.7)], "VEC4", 3, "rotation")
    doc = {"scene": 0, "scenes": [{"nodes": [0, 1, 4]}], "nodes": nodes, "meshes": meshes, "skins": [{"joints": [2, 3], "inverseBindMatrices": ibm_translations(w, [0.0, 1.0])}], "animations": [anim]}
    s = np.zeros(27, bool); s[20:] = True
    return dict(VIEW, path=w.write(tmp_path / "skin_a.gltf", doc), times=TIMES, sentinels=s)


def case_b(tmp_path, seed=2):
    rng = np.random.default_rng(seed); w = Writer(); n = 12; P, N, T, I = strip(rng, n); J, W = blend_weights(P)
    targets = [{"POSITION": rng.uniform(-0.2, 0.2, (n, 3)), "NORMAL": rng.uniform(-0.6, 0.6, (n, 3)), "TANGENT": rng.uniform(-0.6, 0.6, (n, 3))} for _ in range(2)]
    targets[1]["NORMAL"][:3] = 0.0; targets[0]["NORMAL"][:3] = 0.0      # (three vertices no target moves the normal of: they keep the bind normal into the skin)
    anim = {"samplers": [], "channels": []}
    nodes = [{"name": "bar", "mesh": 0, "skin": 0, "translation": [0.5, 0.0, 0.0], "scale": [1.5, 1.0, 1.0]}, {"name": "j0", "children": [2]}, {"name": "j1", "translation": [0.0, 1.0, 0.0]}]
    sampler(w, anim, [0.0, 1.0, 2.0], [quat((0, 0, 1), 0.0), quat((0, 0, 1), -0.9), quat((0, 1, 0), 0.4)], "VEC4", 2, "rotation")
    sampler(w, anim, [0.0, 1.0, 2.0], [0.0, 0.0, 1.0, 0.25, 0.5, 0.75], "SCALAR", 0, "weights")
    doc = {"scene": 0, "scenes": [{"nodes": [0, 1]}], "nodes": nodes, "meshes": [{"primitives": [primitive(w, P, N, T, I, J, W, targets=targets)], "weights": [0.1, 0.2]}],
           "skins": [{"joints": [1, 2], "inverseBindMatrices": ibm_translations(w, [0.0, 1.0])}], "animations": [anim]}
    return dict(VIEW, path=w.write(tmp_path / "skin_b.gltf", doc), times=TIMES, sentinels=np.zeros(n, bool))


def case_c(tmp_path, n=1061, joints=70, seed=3, surround=None, external=False):
    """surround: a scene dict's worth of static triangles is not needed by the tests; tools/skinning_ab.py passes (positions, indices) of static geometry to put around the strip"""
    rng = np.random.default_rng(seed); w = Writer(); P, N, T, I = strip(rng, n)
    J = np.stack([rng.permutation(joints)[:4] for _ in range(n)]) if n <= 4096 else rng.integers(0, joints, (n, 4))
    W = rng.uniform(0.05, 1.0, (n, 4)); W = (W / W.sum(1, keepdims=True)).astype(np.float32)
    ys = np.linspace(0.0, 2.0, joints)
    nodes = [{"name": "strip", "mesh": 0, "skin": 0, "translation": [0.5, 0.0, 0.0]}, {"name": "rig", "children": list(range(2, 2 + joints))}]
    nodes += [{"name": "j%d" % k, "translation": [0.0, float(ys[k]), 0.0]} for k in range(joints)]
    anim = {"samplers": [], "channels": []}
    for k in range(0, joints, 7): sampler(w, anim, [0.0, 1.0, 2.0], [quat((0, 0, 1), 0.0), quat((0.2 * k, 1, 1), 0.3 + 0.01 * k), quat((1, 0, 0), -0.4)], "VEC4", 2 + k, "rotation")
    sampler(w, anim, [0.0, 2.0], [[0, 0, 0], [0.3, 0.1, -0.2]], "VEC3", 1, "translation")
    meshes = [{"primitives": [primitive(w, P, N, T, I, J, W)]}]; roots = [0, 1]
    if surround is not None:
        Ps, Is = surround; Ns = np.zeros_like(Ps); Ns[:, 1] = 1; Ts = np.zeros((len(Ps), 4), np.float32); Ts[:, 0] = 1; Ts[:, 3] = 1
        meshes.append({"primitives": [primitive(w, Ps, Ns, Ts, Is)]}); nodes.append({"name": "static", "mesh": 1}); roots.append(len(nodes) - 1)
    doc = {"scene": 0, "scenes": [{"nodes": roots}], "nodes": nodes, "meshes": meshes, "skins": [{"joints": list(range(2, 2 + joints)), "inverseBindMatrices": ibm_translations(w, ys)}], "animations": [anim]}
    s = np.zeros(n + (0 if surround is None else len(surround[0])), bool); s[n:] = True
    return dict(VIEW, path=w.write(tmp_path / ("skin_c_%d.gltf" % n), doc, external=external), times=TIMES, sentinels=s)


def case_d(tmp_path, seed=4):
    rng = np.random.default_rng(seed); w = Writer(); n = 9; P, N, T, I = strip(rng, n)
    J = np.zeros((n, 4), np.uint8); W = np.zeros((n, 4), np.float32)
    J[:, 0] = 0; J[:, 1] = 1; W[:, 0] = 0.5; W[:, 1] = 0.5                    # ordinary vertices: joints 0 and 1
    W[0] = 0.0                                                                 # all four weights 0: keeps the bind pose
    J[1] = (0, 9, 1, 200); W[1] = (0.25, 0.25, 0.25, 0.25)                     # joints 9 and 200 are beyond the palette of 4: skipped, the rest is not renormalised
    J[2] = (2, 0, 0, 0); W[2] = (1.0, 0, 0, 0)                                 # joint 2 alone: its scale is 0 on one axis at t = 1 — no normal term there, the position still posed
    J[3] = (2, 1, 0, 0); W[3] = (0.5, 0.5, 0, 0)                               # joint 2 and an ordinary joint
    J[4] = (0, 3, 0, 0); W[4] = (0.5, 0.5, 0, 0); N[4] = (1.0, 0.0, 0.0)       # joint 3 is joint 0 turned by pi about Z (exactly diag(-1, -1, 1)): the normal sums to zero length
    nodes = [{"name": "mesh", "mesh": 0, "skin": 0}, {"name": "j0", "children": [2, 3, 4]}, {"name": "j1", "translation": [0.0, 1.0, 0.0]}, {"name": "j2", "translation": [0.0, 0.5, 0.0]},
             {"name": "j3", "rotation": [0.0, 0.0, 1.0, 0.0]}]
    anim = {"samplers": [], "channels": []}
    sampler(w, anim, [0.0, 1.0, 2.0], [quat((0, 0, 1), 0.0), quat((0, 0, 1), 0.8), quat((0, 1, 1), 0.5)], "VEC4", 2, "rotation")
    sampler(w, anim, [0.0, 1.0, 2.0], [[1, 1, 1], [1, 0, 1], [1, 0.5, 2]], "VEC3", 3, "scale")
    M = np.tile(np.eye(4, dtype=np.float32), (4, 1, 1)); M[1, 3, 1] = -1.0; M[2, 3, 1] = -0.5
    doc = {"scene": 0, "scenes": [{"nodes": [0, 1]}], "nodes": nodes, "meshes": [{"primitives": [primitive(w, P, N, T, I, J, W)]}],
           "skins": [{"joints": [1, 2, 3, 4], "inverseBindMatrices": w.add(M.reshape(-1, 16), "MAT4")}], "animations": [anim]}
    return dict(VIEW, path=w.write(tmp_path / "skin_d.gltf", doc), times=TIMES, sentinels=np.zeros(n, bool))


def case_e(tmp_path, seed=5):
    rng = np.random.default_rng(seed); w = Writer(); sizes = (5, 67, 6, 130, 7); deformed = (1, 3)
    meshes, nodes, s = [], [], []
    for k, n in enumerate(sizes):
        P, N, T, I = strip(rng, n)
        if k in deformed: J, W = blend_weights(P); meshes.append({"primitives": [primitive(w, P, N, T, I, J, W)]}); nodes.append({"name": "m%d" % k, "mesh": k, "skin": 0, "translation": [k - 2.0, 0.0, 0.0], "scale": [1.0, 1.0 + 0.1 * k, 1.0]})
        else: meshes.append({"primitives": [primitive(w, P, N, T, I)]}); nodes.append({"name": "m%d" % k, "mesh": k, "translation": [k - 2.0, 0.0, 0.0]})
        s += [k not in deformed] * n
    nodes += [{"name": "j0", "children": [6]}, {"name": "j1", "translation": [0.0, 1.0, 0.0]}]
    anim = {"samplers": [], "channels": []}
    sampler(w, anim, [0.0, 1.0, 2.0], [quat((0, 0, 1), 0.0), quat((0, 0, 1), 1.1), quat((1, 0, 0), 0.6)], "VEC4", 6, "rotation")
    doc = {"scene": 0, "scenes": [{"nodes": [0, 1, 2, 3, 4, 5]}], "nodes": nodes, "meshes": meshes, "skins": [{"joints": [5, 6], "inverseBindMatrices": ibm_translations(w, [0.0, 1.0])}], "animations": [anim]}
    return dict(VIEW, path=w.write(tmp_path / "skin_e.gltf", doc), times=TIMES, sentinels=np.array(s))


def bind_streams(path):
    """(positions float32 [V, 3], normals uint32 [V], tangents uint32 [V]) of the file's bind pose — what pt_load_scene_gltf uploads: the streams of a copy of the file without
    its skins and morph targets"""
    import rtxpt_amd as pt
    doc = json.loads(path.read_text()); doc.pop("skins", None); doc.pop("animations", None)
    for n in doc["nodes"]: n.pop("skin", None)
    for m in doc["meshes"]:
        m.pop("weights", None)
        for pr in m["primitives"]: pr.pop("targets", None)
    q = path.with_name(path.stem + "_bind.gltf"); q.write_text(json.dumps(doc))
    a = pt.GltfAnimation(q); P = a.positions(0.0); N, T = a.normals(0.0); a.close()
    return P, N, T


def make(name, tmp_path):
    return {"A": case_a, "B": case_b, "C": case_c, "D": case_d, "E": case_e}[name](tmp_path)
