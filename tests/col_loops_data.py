"""Inputs of the column-loop tests (test_col_loops_cpu.py, test_gpu_col_loops.py).

Per-rule array loops of the specialized kernels read their elements from path columns
(kvjitgen.cpp ColLoop): an existence anchor over a root-path array from the rows of that array's
family, a loop nested in a loop element from the rows of a nested family (kvdevtypes.h), whose
rows per parent row are the longest nested array among the row's 64 lanes.

Eight single-rule policies:

* ports-exist: spec.containers[].=(ports)[].containerPort, the nested loop;
* volumes-any, volumes-cache: spec.^(volumes)[].name, the existence anchor over a root array
  (two rules of one form: existence anchors never join a rule group, so each runs its own loop);
* proto-0..2: spec.containers[].=(ports)[].protocol != P<k>, three rules of one form that differ
  by one constant: a rule group, the nested loop inside it;
* both: spec.containers[].name (the fused containers loop) and .=(ports)[].containerPort (the
  nested loop) of the same container;
* port-name: spec.containers[].=(ports)[].=(name), a second column of the nested family.

325 Pods (256 + 64 + 5: a full workgroup of four waves, a full wave and a partial one; the first
71, 64 + 7, are the small batch). Container counts, the form of each container's ports, the form
of each port and the volumes cycle with different periods, so that within a wave neighbouring
lanes differ in nested length and the row count of a parent row is another lane's maximum.
"""
N_RES = 325
N_SMALL = 71
RULES = ("ports-exist", "volumes-any", "volumes-cache", "proto-0", "proto-1", "proto-2", "both", "port-name")

# ports of a container: absent, empty, one, three elements, or not an array
PORTS_KINDS = ("absent", "one", "three", "empty", "three", "notarr", "one", "absent", "three", "one", "notarr_map")
# a port: a map with its leaves, not a map, or a map whose containerPort is absent / null / an array
PORT_KINDS = ("ok", "ok", "notmap", "noleaf", "ok", "null", "arrleaf", "ok", "low", "proto")
VOLUME_KINDS = ("absent", "empty", "notarr", "first", "last", "none", "notmap_then_hit", "arrleaf", "cache", "single")


def _rule(name, pattern):
    return {"name": name, "match": {"resources": {"kinds": ["Pod"]}}, "validate": {"pattern": pattern}}


def policies():
    rules = [
        _rule("ports-exist", {"spec": {"containers": [{"=(ports)": [{"containerPort": "*"}]}]}}),
        _rule("volumes-any", {"spec": {"^(volumes)": [{"name": "data"}]}}),
        _rule("volumes-cache", {"spec": {"^(volumes)": [{"name": "cache"}]}}),
    ]
    rules += [_rule(f"proto-{k}", {"spec": {"containers": [{"=(ports)": [{"protocol": f"!P{k}"}]}]}}) for k in range(3)]
    rules += [
        _rule("both", {"spec": {"containers": [{"name": "c*", "=(ports)": [{"containerPort": ">1024"}]}]}}),
        _rule("port-name", {"spec": {"containers": [{"=(ports)": [{"=(name)": "p*"}]}]}}),
    ]
    assert tuple(r["name"] for r in rules) == RULES
    # (one policy per rule: the oracle's per-pair path lookup evaluates one whole policy)
    return [{"apiVersion": "kyverno.io/v1", "kind": "ClusterPolicy", "metadata": {"name": r["name"]},
             "spec": {"validationFailureAction": "audit", "background": True, "rules": [r]}} for r in rules]


# lanes (of every wave) with three containers and ports only in the second / only in the last one
ONLY_SECOND, ONLY_LAST = (5, 37), (6, 38)


def n_containers(i):
    """0..3 containers; None: no containers key"""
    if i % 64 in ONLY_SECOND + ONLY_LAST:
        return 3
    return (None, 1, 2, 3, 0, 3, 2, 1, 3)[i % 9]


def ports_kind(i, c):
    lane = i % 64
    if lane in ONLY_SECOND:
        return "three" if c == 1 else "absent"
    if lane in ONLY_LAST:
        return "one" if c == 2 else "absent"
    return PORTS_KINDS[(i + 4 * c) % len(PORTS_KINDS)]


def port_kind(i, c, e):
    return PORT_KINDS[(i // 3 + 3 * c + 7 * e) % len(PORT_KINDS)]


def volumes_kind(i):
    return VOLUME_KINDS[(i + i // 64) % len(VOLUME_KINDS)]


def _port(kind, e):
    if kind == "notmap":
        return "http"
    p = {"containerPort": 8080 + e, "protocol": "TCP", "name": f"p{e}"}
    if kind == "noleaf":
        del p["containerPort"]
        del p["name"]
    elif kind == "null":
        p["containerPort"] = None
        p["name"] = None
    elif kind == "arrleaf":
        p["containerPort"] = [8080, 9090]
        p["name"] = ["p0", "q"]
    elif kind == "low":
        p["containerPort"] = 80
        p["name"] = "web"
        del p["protocol"]
    elif kind == "proto":
        p["protocol"] = f"P{e % 3}"
    return p


def _ports(i, c):
    kind = ports_kind(i, c)
    if kind == "absent":
        return None
    if kind == "notarr":
        return "none"
    if kind == "notarr_map":
        return {"containerPort": 1}
    n = {"empty": 0, "one": 1, "three": 3}[kind]
    return [_port(port_kind(i, c, e), e) for e in range(n)]


def _volumes(kind):
    named = lambda *names: [{"name": n, "emptyDir": {}} for n in names]
    return {"empty": [], "notarr": "data", "first": named("data", "a", "b"), "last": named("a", "b", "data"),
            "none": [{"name": "a"}, {"name": None}, {"emptyDir": {}}], "notmap_then_hit": ["data", {"name": "data"}],
            "arrleaf": [{"name": ["data"]}, {"name": "b"}], "cache": named("cache"), "single": named("data")}[kind]


def resources():
    out = []
    for i in range(N_RES):
        spec = {}
        nc = n_containers(i)
        if nc is not None:
            cs = []
            for c in range(nc):
                ct = {"name": f"c{c}" if (i + c) % 11 else f"x{c}", "image": "reg.io/app:v1"}
                ports = _ports(i, c)
                if ports is not None:
                    ct["ports"] = ports
                cs.append(ct if (i + c) % 29 or i % 64 in ONLY_SECOND + ONLY_LAST else "not-a-map")
            spec["containers"] = cs
        vk = volumes_kind(i)
        if vk != "absent":
            spec["volumes"] = _volumes(vk)
        out.append({"apiVersion": "v1", "kind": "Pod", "metadata": {"name": f"pod-{i}", "namespace": f"ns-{i % 5}"},
                    "spec": spec})
    return out


def path_indices(path):
    """(template, indices) of a failing path: its array indices in order, and the path with
    each replaced by '#'"""
    segs = path.split("/")
    idx = [int(s) for s in segs if s.isdigit()]
    return "/".join("#" if s.isdigit() else s for s in segs), idx
