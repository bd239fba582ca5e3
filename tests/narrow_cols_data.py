"""Inputs of the narrow path-column tests (test_narrow_cols_cpu.py, test_gpu_narrow_cols.py).

Four single-rule policies: a root leaf, an element leaf under spec.containers[], a nested
element leaf under ports[], and a wildcard-key pattern under metadata.labels (which reads the
labels map's own node index, so that column stays wide). 320 hand-built Pods: one full
workgroup of the specialized kernels plus a partial one. The value at the root leaf and at
the element leaf cycles through the eight LEAF_KINDS; container counts cycle 0, 1, 2, 3 within
each 64-resource group, so a wave's element rows are padded past the lanes with fewer elements.
"""

N_RES = 320

# the value at a leaf position, by kind (None: the key is absent)
LEAF_KINDS = ("match", "nomatch", "null", "map", "empty_array", "array_pass", "array_fail", "absent")


def _policy(name, pattern):
    return {"apiVersion": "kyverno.io/v1", "kind": "ClusterPolicy", "metadata": {"name": name},
            "spec": {"validationFailureAction": "audit", "background": True,
                     "rules": [{"name": name, "match": {"resources": {"kinds": ["Pod"]}},
                                "validate": {"pattern": pattern}}]}}


def policies():
    return [
        _policy("root-leaf", {"spec": {"schedulerName": "good*"}}),
        _policy("elem-leaf", {"spec": {"containers": [{"imagePullPolicy": "Always"}]}}),
        _policy("nested-leaf", {"spec": {"containers": [{"=(ports)": [{"protocol": "TCP"}]}]}}),
        _policy("label-wild", {"metadata": {"labels": {"a*": "?*"}}}),
    ]


def _leaf(kind, good, bad):
    return {"match": good, "nomatch": bad, "null": None, "map": {"k": good}, "empty_array": [],
            "array_pass": [good, good], "array_fail": [good, bad, good]}[kind]


def root_kind(i):
    return LEAF_KINDS[i % 8]


def elem_kind(i, c):
    # (a resource's containers mostly match, so that one odd element decides the rule)
    return LEAF_KINDS[(i // 8 + c) % 8] if c == (i // 4) % 3 else "match"


def n_containers(i):
    return (i % 64) % 4


def resources():
    out = []
    for i in range(N_RES):
        spec = {}
        rk = root_kind(i)
        if rk != "absent":
            spec["schedulerName"] = _leaf(rk, "good-sched", "other")
        cs = []
        for c in range(n_containers(i)):
            ct = {"name": f"c{c}", "image": f"img-{c}:v1"}
            ek = elem_kind(i, c)
            if ek != "absent":
                ct["imagePullPolicy"] = _leaf(ek, "Always", "Never")
            if (i + c) % 3:
                ct["ports"] = [{"containerPort": 80 + p, "protocol": "UDP" if (i + c + p) % 7 == 0 else "TCP"}
                               for p in range(1 + (i + c) % 2)]
            cs.append(ct)
        # (a Pod without the containers key, and with an empty list)
        if n_containers(i) or i % 8 == 0:
            spec["containers"] = cs
        labels = [{"app": "web"}, {"tier": "db"}, {"app": "", "zone": "z"}, None][i % 4]
        md = {"name": f"pod-{i}", "namespace": f"ns-{i % 5}"}
        if labels is not None:
            md["labels"] = labels
        out.append({"apiVersion": "v1", "kind": "Pod", "metadata": md, "spec": spec})
    return out
