"""Inputs of the hoisted leaf-word tests (test_hoist_words_cpu.py, test_gpu_hoist_words.py).

46 single-rule policies whose rules fuse into one block of one specialized kernel and share its hoist
regions (kvjitgen.cpp HoistTable):

* 40 image-glob rules on spec.containers[].image: one rule group, whose 40 members take 40
  consecutive bits of the leaf's table words, so that one cell needs two words;
* one rule each on spec.containers[].imagePullPolicy and spec.containers[].workingDir: with the
  image that is three leaf cells and four leaf words in the region of the containers loop;
* one rule each on the root leaves spec.schedulerName, spec.priorityClassName and spec.dnsPolicy
  (the root region);
* a wildcard-key rule on metadata.labels, which reads the labels map's own node index and so
  keeps one column wide while the leaf columns are narrow.

320 Pods: one full workgroup of the specialized kernels (four waves) and a partial one. The value
at each of the six leaves cycles through narrow_cols_data.LEAF_KINDS, offset differently per leaf;
a per-wave rule then says where the array kinds may stay (elsewhere a scalar kind takes their
place), so that the array fix-up of a region (one wave-uniform test, then per lane and leaf) meets:

* wave 0: no array at any hoisted leaf (the fix-up is skipped);
* wave 1: a single lane with an array, at one element leaf;
* wave 2: arrays at different leaves on different lanes, at most one leaf per lane;
* wave 3: every array the cycles give, and lanes with two array leaves in one region (image and
  workingDir of one container; schedulerName and dnsPolicy);
* wave 4 (the partial workgroup): a single lane with an array, at one root leaf.

Arrays have 0 to 3 elements, fail at the first or at the last element, hold a null element or a
nested array. Container counts cycle 0, 0, 0, 1, 1, 1, ... 3, 3, 3 within each wave.
"""
from narrow_cols_data import LEAF_KINDS

N_RES = 320
N_IMAGE = 40

LEAVES = ("image", "imagePullPolicy", "workingDir", "schedulerName", "priorityClassName", "dnsPolicy")
ELEM_LEAVES, ROOT_LEAVES = LEAVES[:3], LEAVES[3:]
OFFSET = {"image": 0, "imagePullPolicy": 3, "workingDir": 5, "schedulerName": 1, "priorityClassName": 4, "dnsPolicy": 6}
ARRAY_KINDS = ("empty_array", "array_pass", "array_fail")
SCALAR_KINDS = tuple(k for k in LEAF_KINDS if k not in ARRAY_KINDS)

# (passing value, failing value) of the single-rule leaves; the image's depend on the resource
VALUES = {"imagePullPolicy": ("Always", "Never"), "workingDir": ("/app/bin", "/tmp"),
          "schedulerName": ("good-sched", "other"), "priorityClassName": ("high-prio", "low"),
          "dnsPolicy": ("ClusterFirst", "Default")}


def _rule(name, pattern):
    return {"name": name, "match": {"resources": {"kinds": ["Pod"]}}, "validate": {"pattern": pattern}}


def policies():
    rules = [_rule(f"image-{k:02d}", {"spec": {"containers": [{"image": f"!*-b{k:02d}:*"}]}}) for k in range(N_IMAGE)]
    rules += [
        _rule("pull", {"spec": {"containers": [{"imagePullPolicy": "Always"}]}}),
        _rule("workdir", {"spec": {"containers": [{"workingDir": "/app*"}]}}),
        _rule("sched", {"spec": {"schedulerName": "good*"}}),
        _rule("prio", {"spec": {"priorityClassName": "high*"}}),
        _rule("dns", {"spec": {"dnsPolicy": "ClusterFirst"}}),
        _rule("label-wild", {"metadata": {"labels": {"a*": "?*"}}}),
    ]
    # (one policy per rule: the oracle's per-pair path lookup evaluates one whole policy)
    return [{"apiVersion": "kyverno.io/v1", "kind": "ClusterPolicy", "metadata": {"name": r["name"]},
             "spec": {"validationFailureAction": "audit", "background": True, "rules": [r]}} for r in rules]


def n_containers(i):
    return ((i % 64) // 3) % 4


def _cycle(leaf, i, c):
    return LEAF_KINDS[(i + OFFSET[leaf] + 3 * c) % 8]


# lanes the per-wave rules single out
W1_LANE, W3_LANE, W4_LANE = 17, 11, 6


def leaf_kind(leaf, i, c=0):
    """kind of the value at `leaf` of resource i (an element leaf: of its container c)"""
    w, lane = i // 64, i % 64
    k = _cycle(leaf, i, c)
    scalar = SCALAR_KINDS[(i + c + OFFSET[leaf]) % len(SCALAR_KINDS)]
    if w == 0:
        return scalar if k in ARRAY_KINDS else k
    if w == 1:
        if lane == W1_LANE and leaf == "imagePullPolicy" and c == 0:
            return "array_fail"
        return scalar if k in ARRAY_KINDS else k
    if w == 2:  # arrays only at leaf (lane mod 6) of the lane, and there only in container 0
        if k in ARRAY_KINDS and not (LEAVES[lane % 6] == leaf and c == 0):
            return scalar
        return k
    if w == 3:
        if lane == W3_LANE and c == 0 and leaf in ("image", "workingDir"):
            return "array_fail" if leaf == "image" else "array_pass"
        if lane == W3_LANE and leaf in ("schedulerName", "dnsPolicy"):
            return "array_pass" if leaf == "dnsPolicy" else "empty_array"
        return k
    if lane == W4_LANE and leaf == "priorityClassName":
        return "array_pass"
    return scalar if k in ARRAY_KINDS else k


def _value(kind, good, bad, v):
    """the value of `kind`; v picks the form of an array"""
    if kind == "array_pass":
        return [[good], [good, good], [good, good, good]][v % 3]
    if kind == "array_fail":  # fails first, fails last, a null element, a nested array
        return [[bad, good, good], [good, good, bad], [good, None], [good, [good]], [bad]][v % 5]
    return {"match": good, "nomatch": bad, "null": None, "map": {"k": good}, "empty_array": []}[kind]


def _image_values(i, c):
    # passes every image rule / fails image rule (i + c) mod 40 alone
    return f"reg.io/app-ok{(i + c) % 4}:v1", f"reg.io/app-b{(i + c) % N_IMAGE:02d}:v1"


def resources():
    out = []
    for i in range(N_RES):
        spec = {}
        for leaf in ROOT_LEAVES:
            k = leaf_kind(leaf, i)
            if k != "absent":
                spec[leaf] = _value(k, *VALUES[leaf], i // 8)
        cs = []
        for c in range(n_containers(i)):
            ct = {"name": f"c{c}"}
            for leaf in ELEM_LEAVES:
                k = leaf_kind(leaf, i, c)
                if k != "absent":
                    good, bad = _image_values(i, c) if leaf == "image" else VALUES[leaf]
                    ct[leaf] = _value(k, good, bad, i // 8 + c)
            cs.append(ct)
        if n_containers(i) or i % 8 == 0:  # (a Pod without the containers key, and with an empty list)
            spec["containers"] = cs
        labels = [{"app": "web"}, {"tier": "db"}, {"app": "", "zone": "z"}, None][i % 4]
        md = {"name": f"pod-{i}", "namespace": f"ns-{i % 5}"}
        if labels is not None:
            md["labels"] = labels
        out.append({"apiVersion": "v1", "kind": "Pod", "metadata": md, "spec": spec})
    return out
