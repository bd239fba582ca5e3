"""Batch API over the C ABI: compile a policy set once, ingest resources once,
evaluate every (resource, rule) pair on a MI355X.

This is the batch form of ``engine.Validate`` (reference
``pkg/engine/validation.go:26``): statuses use ``response.RuleStatus`` codes
(``pkg/engine/response/status.go:14-28``) plus ``NOMATCH`` (no RuleResponse)
and ``CPU`` (the pair needs the reference CPU engine: context, deny, foreach,
``{{ }}`` variables other than ``request.object`` paths, or preconditions outside
the device forms). Preconditions that are an ``any`` / ``all`` (or old list) of
Equal(s), NotEqual(s), the In family and the four numeric comparisons, each with
``request.object`` variables on one side and a constant scalar or list on the other,
are evaluated on the device (``kv_precond_kernel``): a pair whose preconditions do
not hold is ``SKIP`` (``Result.precond_message``), one they cannot decide there (a
map or array operand) is ``CPU``. ``PolicySet(..., deny=True)`` (``KV_COMPILE_DENY``, opt-in)
also evaluates ``validate.deny`` rules whose conditions are of those forms on the device
(``kv_deny_kernel``): ``FAIL`` when the conditions hold, ``PASS`` when they do not, ``ERROR`` when
a variable does not resolve (``Result.deny_message``). ``PolicySet(..., foreach=True)``
(``KV_COMPILE_FOREACH``, opt-in) evaluates single-entry ``validate.foreach`` rules with a ``deny``
block over ``{{element...}}`` the same way, one lane per list element (``kv_foreach_elem_kernel``):
the first ``FAIL`` / ``ERROR`` element decides (``Result.foreach_element``), else ``PASS`` when an
element passed, else ``SKIP`` "rule skipped" (``Result.foreach_message``).
``PolicySet(..., foreach=True, foreach_pattern=True)`` (``KV_COMPILE_FOREACH_PATTERN``, opt-in) also
evaluates entries that carry a ``pattern``: the pattern is matched per element with the element as
the whole resource (``kv_foreach_pat_kernel``); the deciding element's failing path and pattern
error are ``Result.foreach_path`` / ``Result.foreach_error_message``.
``PolicySet(..., foreach=True, foreach_entries=True)`` (``KV_COMPILE_FOREACH_ENTRIES``, opt-in) also
takes ``validate.foreach`` rules of 2 to 16 such entries (``kv_foreach_chain_kernel`` walks the
entries' rows in order); ``Result.foreach_entry`` names the deciding entry.
"""
from __future__ import annotations

import ctypes
import json
from dataclasses import dataclass

import numpy as np

from . import _native
from ._native import RuleInfo, check, lib, new_err

PASS, FAIL, WARN, ERROR, SKIP, NOMATCH, CPU = range(7)
STATUS_NAMES = ["pass", "fail", "warn", "error", "skip", "nomatch", "cpu"]

MODE_STATUS, MODE_ERRORS, MODE_COUNTS, MODE_SCOPES = 1, 2, 4, 8
COMPILE_SPECIALIZE, COMPILE_DENY, COMPILE_FOREACH, COMPILE_FOREACH_PATTERN = 1, 2, 4, 8
COMPILE_FOREACH_ENTRIES = 16
COMPILE_FOREACH_ANYPATTERN = 32
COMPILE_FOREACH_PATVARS = 64
ROUTE_GPU, ROUTE_CPU, ROUTE_NORESPONSE, ROUTE_CONSTANT = range(4)


def condition_eval(condition: dict) -> bool:
    """``variables.Evaluate`` of one already-substituted condition ``{"key", "operator", "value"}``
    (numbers as float64) by the library's host evaluator (``kv_condition_eval``; no GPU). Raises
    ``ValueError`` for operands outside the device scope (a map, a list key, Duration* operators)."""
    raw = json.dumps(condition, ensure_ascii=False).encode("utf-8")
    out = ctypes.c_int()
    rc = lib().kv_condition_eval(raw, len(raw), ctypes.byref(out))
    if rc != 0:
        raise ValueError(f"kv_condition_eval: code {rc}")
    return bool(out.value)


def _dumps(x) -> bytes:
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    if isinstance(x, str):
        return x.encode("utf-8")
    return json.dumps(x, ensure_ascii=False, separators=(",", ":")).encode("utf-8")


@dataclass
class Rule:
    index: int
    policy: int
    policy_name: str
    name: str
    route: int
    route_reason: str
    message: str
    any_pattern: bool
    const_status: int
    const_message: str
    deny: bool = False  # a validate.deny rule evaluated on the device (PolicySet(deny=True))
    foreach: bool = False  # a validate.foreach rule evaluated on the device (PolicySet(foreach=True))
    foreach_pattern: bool = False  # ... whose entry carries a pattern (PolicySet(foreach_pattern=True))
    foreach_entries: int = 0  # ... of several entries: their number (PolicySet(foreach_entries=True)), else 0
    foreach_anypattern: int = 0  # ... whose one entry carries an anyPattern: its alternatives (PolicySet(foreach_anypattern=True))
    foreach_patvars: bool = False  # ... with variable strings in an entry's pattern (PolicySet(foreach_patvars=True))


class PolicySet:
    """Compiled policies (``kv_compile``). Input: list of policy dicts or JSON text.

    ``specialize=True`` also lowers every rule to specialized gfx950 kernels
    (hiprtc, at construction); evaluation then runs those instead of the
    bytecode interpreter. ``jit_info`` reports their build cost.

    ``deny=True`` (``KV_COMPILE_DENY``, opt-in) routes ``validate.deny`` rules of the device forms
    to the GPU: any / all (or old list) conditions as the preconditions accept them, over
    ``request.object`` variables. A pair is ``FAIL`` when the conditions hold, ``PASS`` when they
    do not, ``ERROR`` when a variable does not resolve (``Result.deny_message``), ``CPU`` when the
    device cannot decide. Without it every deny rule is CPU-routed, reason ``"deny"``.

    ``foreach=True`` (``KV_COMPILE_FOREACH``, opt-in, independent of ``deny``) routes
    ``validate.foreach`` rules of one entry ``{list, preconditions?, deny}`` to the GPU: ``list`` a
    ``request.object`` path, the conditions over ``{{element...}}`` / ``{{request.object...}}``
    variables. Without it every foreach rule is CPU-routed, reason ``"foreach"``.

    ``foreach_pattern=True`` (``KV_COMPILE_FOREACH_PATTERN``, opt-in, needs ``foreach``) also routes
    entries ``{list, preconditions?, pattern}`` to the GPU: the pattern a map without ``{{ }}``
    variables or a ``metadata`` key. Without it such a rule stays CPU-routed, reason ``"foreach"``.

    ``foreach_entries=True`` (``KV_COMPILE_FOREACH_ENTRIES``, opt-in, needs ``foreach``) also routes
    rules of 2 to 16 entries, each of the forms above, to the GPU. As in the reference, the
    ``{{element...}}`` variables of a later entry read the element merged over the last elements of
    the lists before it. Without it such a rule stays CPU-routed, reason ``"foreach"``.

    ``foreach_anypattern=True`` (``KV_COMPILE_FOREACH_ANYPATTERN``, opt-in, needs ``foreach`` and
    ``foreach_pattern``) also routes entries ``{list, preconditions?, anyPattern}`` to the GPU:
    ``anyPattern`` a list of 1 to 8 maps, each within the limits of a pattern entry. An element
    passes when one alternative matches; ``Result.foreach_alt`` gives every alternative's outcome on
    the deciding element of a FAIL pair. Without it such a rule stays CPU-routed, reason ``"foreach"``.

    ``foreach_patvars=True`` (``KV_COMPILE_FOREACH_PATVARS``, opt-in, needs ``foreach`` and
    ``foreach_pattern``; composes with the other two) also routes entries whose ``pattern`` (or
    ``anyPattern``) holds ``{{element...}}`` / ``{{request.object...}}`` variables in its string
    values. Per element the pattern is substituted first: an unresolved variable makes the element
    ``ERROR`` (``Result.foreach_subst_error``), then the substituted pattern is matched against the
    element. Without it such a rule stays CPU-routed, reason ``"foreach"``.
    """

    def __init__(self, policies, specialize: bool = False, deny: bool = False, foreach: bool = False,
                 foreach_pattern: bool = False, foreach_entries: bool = False, foreach_anypattern: bool = False,
                 foreach_patvars: bool = False):
        L = lib()
        data = _dumps(policies)
        h = ctypes.c_void_p()
        err = new_err()
        flags = ((COMPILE_SPECIALIZE if specialize else 0) | (COMPILE_DENY if deny else 0)
                 | (COMPILE_FOREACH if foreach else 0) | (COMPILE_FOREACH_PATTERN if foreach_pattern else 0)
                 | (COMPILE_FOREACH_ENTRIES if foreach_entries else 0)
                 | (COMPILE_FOREACH_ANYPATTERN if foreach_anypattern else 0)
                 | (COMPILE_FOREACH_PATVARS if foreach_patvars else 0))
        check(L.kv_compile(data, len(data), flags, ctypes.byref(h), ctypes.byref(err)), err)
        self._h = h
        self.specialize = specialize
        self.deny = deny
        self.foreach = foreach
        self.foreach_pattern = foreach_pattern
        self.foreach_entries = foreach_entries
        self.foreach_anypattern = foreach_anypattern
        self.foreach_patvars = foreach_patvars
        np_, nr = ctypes.c_uint32(), ctypes.c_uint32()
        L.kv_policyset_info(h, ctypes.byref(np_), ctypes.byref(nr))
        self.n_policies, self.n_rules = np_.value, nr.value
        self.rules: list[Rule] = []
        for i in range(self.n_rules):
            ri = RuleInfo()
            L.kv_rule_info_get(h, i, ctypes.byref(ri))
            d = lambda b: (b or b"").decode("utf-8")  # noqa: E731
            self.rules.append(Rule(i, ri.policy, d(ri.policy_name), d(ri.name), ri.route, d(ri.route_reason),
                                   d(ri.message), bool(ri.any_pattern), ri.const_status, d(ri.const_message)))
            ds = ctypes.c_uint32()
            L.kv_rule_deny_set(h, i, ctypes.byref(ds))
            self.rules[-1].deny = ds.value != 0
            self.rules[-1].foreach = ri.foreach_set != 0
            on = ctypes.c_uint32()
            L.kv_rule_foreach_pattern(h, i, ctypes.byref(on))
            self.rules[-1].foreach_pattern = on.value != 0
            L.kv_rule_foreach_anypattern(h, i, ctypes.byref(on))
            self.rules[-1].foreach_anypattern = on.value
            L.kv_rule_foreach_patvars(h, i, ctypes.byref(on))
            self.rules[-1].foreach_patvars = on.value != 0
            ch, ne = ctypes.c_uint32(), ctypes.c_uint32()
            L.kv_rule_foreach_chain(h, i, ctypes.byref(ch), ctypes.byref(ne))
            if ch.value:  # (kv_rule_info.foreach_set stays 0 for a rule of several entries)
                self.rules[-1].foreach = True
                self.rules[-1].foreach_entries = ne.value

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                lib().kv_free_policyset(h)
            except Exception:
                pass
            self._h = None

    @property
    def jit_info(self) -> dict:
        nk, cb = ctypes.c_uint32(), ctypes.c_uint64()
        g, c = ctypes.c_double(), ctypes.c_double()
        lib().kv_policyset_jit_info(self._h, ctypes.byref(nk), ctypes.byref(g), ctypes.byref(c), ctypes.byref(cb))
        cw, cn = ctypes.c_uint32(), ctypes.c_uint32()
        lib().kv_policyset_jit_cols(self._h, ctypes.byref(cw), ctypes.byref(cn))
        return {"kernels": nk.value, "gen_ms": g.value, "compile_ms": c.value, "code_bytes": cb.value,
                "cols_wide": cw.value, "cols_narrow": cn.value}

    @property
    def precondition_info(self) -> dict:
        """Preconditions evaluated on the device: interned condition sets, conditions with a
        variable operand and distinct condition strings (``kv_policyset_cond_sets``)."""
        s, c, k = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        lib().kv_policyset_cond_sets(self._h, ctypes.byref(s), ctypes.byref(c), ctypes.byref(k))
        return {"sets": s.value, "conditions": c.value, "strings": k.value}

    @property
    def deny_info(self) -> dict:
        """Deny rules evaluated on the device: interned deny sets, their conditions with a variable
        operand and their distinct condition strings (``kv_policyset_deny_sets``), and per rule
        1 + its deny set, 0 for a rule that is not a device deny rule (``kv_rule_deny_set``)."""
        s, c, k = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        lib().kv_policyset_deny_sets(self._h, ctypes.byref(s), ctypes.byref(c), ctypes.byref(k))
        rule_sets = []
        for i in range(self.n_rules):
            ds = ctypes.c_uint32()
            lib().kv_rule_deny_set(self._h, i, ctypes.byref(ds))
            rule_sets.append(ds.value)
        return {"sets": s.value, "conditions": c.value, "strings": k.value, "rule_sets": rule_sets}

    def deny_fold(self, b: "Batch") -> np.ndarray:
        """u8 [deny sets][n_res]: the deny fold of every deny set over batch ``b`` on the host
        (``kv_batch_deny_fold``, no GPU): what ``kv_deny_kernel`` writes, before match / exclude
        and the preconditions are applied."""
        n_sets = self.deny_info["sets"]
        out = np.zeros((n_sets, b.n_res), dtype=np.uint8)
        for s in range(n_sets):
            rc = lib().kv_batch_deny_fold(self._h, b._h, s, out[s].ctypes.data, b.n_res)
            if rc != 0:
                raise RuntimeError(f"kv_batch_deny_fold: code {rc}")
        return out

    @property
    def foreach_info(self) -> dict:
        """Foreach rules evaluated on the device: interned foreach sets, lists, conditions with a
        variable operand and element-scoped strings (``kv_policyset_foreach_sets``), and per rule
        1 + its foreach set, 0 for a rule that is not a device foreach rule."""
        v = [ctypes.c_uint32() for _ in range(4)]
        lib().kv_policyset_foreach_sets(self._h, *[ctypes.byref(x) for x in v])
        rule_sets = []
        for i in range(self.n_rules):
            fs = ctypes.c_uint32()
            lib().kv_rule_foreach_set(self._h, i, ctypes.byref(fs))
            rule_sets.append(fs.value)
        return {"sets": v[0].value, "lists": v[1].value, "conditions": v[2].value, "strings": v[3].value,
                "rule_sets": rule_sets}

    def foreach_fold(self, b: "Batch") -> tuple[np.ndarray, np.ndarray]:
        """(u8 status, u32 element) [foreach sets][n_res]: the foreach fold of every set over batch
        ``b`` on the host (``kv_batch_foreach_fold``, no GPU), the twin of the two kernels, before
        match / exclude and the rule's preconditions; element 0xFFFFFFFF: no deciding element. The
        rows of pattern sets (``foreach_pattern=True``) stay unset, status 255: their elements are
        walked on the device only."""
        info = self.foreach_info
        n_sets = info["sets"]
        st = np.zeros((n_sets, b.n_res), dtype=np.uint8)
        el = np.full((n_sets, b.n_res), 0xFFFFFFFF, dtype=np.uint32)
        for s in range(n_sets):
            on = ctypes.c_uint32()
            lib().kv_foreach_set_pattern(self._h, s, ctypes.byref(on))
            na = ctypes.c_uint32()
            lib().kv_foreach_set_alternatives(self._h, s, ctypes.byref(na))
            if on.value or na.value:  # (a pattern set or any set, of a rule of one entry or of several)
                st[s] = 255
                continue
            rc = lib().kv_batch_foreach_fold(self._h, b._h, s, st[s].ctypes.data, el[s].ctypes.data, b.n_res)
            if rc != 0:
                raise RuntimeError(f"kv_batch_foreach_fold: code {rc}")
        return st, el

    @property
    def foreach_chain_info(self) -> dict:
        """Foreach rules of several entries (``foreach_entries=True``): the interned chains
        (``kv_policyset_foreach_chains``), per chain the foreach sets of its entries in order
        (``kv_chain_entry_set``, 0-based), and per rule 1 + its chain, 0 for any other rule
        (``kv_rule_foreach_chain``)."""
        n = ctypes.c_uint32()
        lib().kv_policyset_foreach_chains(self._h, ctypes.byref(n))
        rule_chains, entries = [], {}
        for i in range(self.n_rules):
            ch, ne = ctypes.c_uint32(), ctypes.c_uint32()
            lib().kv_rule_foreach_chain(self._h, i, ctypes.byref(ch), ctypes.byref(ne))
            rule_chains.append(ch.value)
            if ch.value:
                entries[ch.value - 1] = ne.value
        chain_sets = []
        for c in range(n.value):
            sets, k = [], 0
            while True:
                s = ctypes.c_uint32()
                if lib().kv_chain_entry_set(self._h, c, k, ctypes.byref(s)) != 0:
                    break
                sets.append(s.value)
                k += 1
            chain_sets.append(sets)
        return {"chains": n.value, "chain_sets": chain_sets, "rule_chains": rule_chains}

    def foreach_chain_fold(self, b: "Batch") -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(u8 status, u32 entry, u32 element) [chains][n_res]: the fold of every chain over batch
        ``b`` on the host (``kv_batch_foreach_chain_fold``, no GPU), the twin of the entry kernels and
        ``kv_foreach_chain_kernel``; entry / element 0xFFFFFFFF: none decided. The rows of chains
        with a pattern entry stay unset, status 255."""
        n = self.foreach_chain_info["chains"]
        st = np.zeros((n, b.n_res), dtype=np.uint8)
        en = np.full((n, b.n_res), 0xFFFFFFFF, dtype=np.uint32)
        el = np.full((n, b.n_res), 0xFFFFFFFF, dtype=np.uint32)
        for c in range(n):
            rc = lib().kv_batch_foreach_chain_fold(self._h, b._h, c, st[c].ctypes.data, en[c].ctypes.data,
                                                   el[c].ctypes.data, b.n_res)
            if rc == -1:
                st[c] = 255
            elif rc != 0:
                raise RuntimeError(f"kv_batch_foreach_chain_fold: code {rc}")
        return st, en, el

    def foreach_subst(self, b: "Batch", fset: int, res: int, elem: int) -> tuple[int, str | None]:
        """Diagnostics: the substitution verdict of element ``elem`` of resource ``res`` under the pattern strings of
        foreach set ``fset`` (``foreach_patvars=True``) on the host (``kv_batch_foreach_subst``, no GPU;
        the function the kernels run): (0 | ERROR | CPU, the error text of an ERROR)."""
        code = ctypes.c_uint32()
        cap = 1024
        while True:
            buf = ctypes.create_string_buffer(cap)
            n = lib().kv_batch_foreach_subst(self._h, b._h, fset, res, elem, ctypes.byref(code), buf, cap)
            if n < 0:
                raise RuntimeError(f"kv_batch_foreach_subst: code {n}")
            if n < cap:
                return code.value, (buf.raw[:n].decode("utf-8", "replace") if code.value == ERROR else None)
            cap = n + 1

    def foreach_tables(self, b: "Batch") -> bytes:
        """The per-batch foreach tables of ``b`` as the device receives them, as bytes
        (``kv_batch_foreach_tables``; diagnostics, no GPU)."""
        p, ln = ctypes.c_void_p(), ctypes.c_size_t()
        rc = lib().kv_batch_foreach_tables(self._h, b._h, ctypes.byref(p), ctypes.byref(ln))
        if rc != 0:
            raise RuntimeError(f"kv_batch_foreach_tables: code {rc}")
        try:
            return ctypes.string_at(p.value, ln.value)
        finally:
            lib().kv_free_buffer(p)

    def foreach_chain_message(self, b: "Batch", chain: int, res: int) -> str | None:
        """What ``Result.foreach_message`` gives for resource ``res`` of chain ``chain`` where the fold
        decides the pair, from the host fold (``kv_batch_foreach_chain_message``, no GPU): the ERROR
        text of a deny entry, "rule skipped" for a SKIP, else None."""
        cap = 256
        while True:
            buf = ctypes.create_string_buffer(cap)
            n = lib().kv_batch_foreach_chain_message(self._h, b._h, chain, res, buf, cap)
            if n <= 0:
                return None
            if n < cap:
                return buf.raw[:n].decode("utf-8")
            cap = n + 1

    def policy_rules(self, policy: int) -> list[Rule]:
        return [r for r in self.rules if r.policy == policy]


class Batch:
    """Ingested resources (``kv_ingest``): list of dicts, JSON array text or NDJSON."""

    def __init__(self, policyset: PolicySet, resources, namespace_labels: dict | None = None):
        L = lib()
        if isinstance(resources, (list, tuple)):
            data = b"\n".join(_dumps(r) for r in resources)
        else:
            data = _dumps(resources)
        ns = _dumps(namespace_labels) if namespace_labels else None
        h = ctypes.c_void_p()
        err = new_err()
        check(L.kv_ingest(policyset._h, data, len(data), ns, ctypes.byref(h), ctypes.byref(err)), err)
        self._h = h
        self.policyset = policyset
        n, b = ctypes.c_uint64(), ctypes.c_uint64()
        L.kv_batch_info(h, ctypes.byref(n), ctypes.byref(b))
        self.n_res, self.store_bytes = n.value, b.value

    @property
    def transfer_bytes(self) -> int:
        """Bytes the store crosses PCIe in (kv_batch_transfer_bytes: 8-byte transfer cells)."""
        n = ctypes.c_uint64()
        lib().kv_batch_transfer_bytes(self._h, ctypes.byref(n))
        return n.value

    @property
    def namespaces(self) -> list[str]:
        """Batch namespace table: index = scope of per-scope counts ("" = cluster scope)."""
        n = ctypes.c_uint32()
        lib().kv_batch_namespaces(self._h, ctypes.byref(n))
        return [lib().kv_batch_namespace(self._h, i).decode("utf-8") for i in range(n.value)]

    def close(self) -> None:
        """Free the host batch now (e.g. once a parts session holds its device copy)."""
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                lib().kv_free_batch(h)
            except Exception:
                pass
            self._h = None

    def __del__(self):
        self.close()


class _ResultHandle:
    """Owner of one kv_result handle: freed when the Result and every copy=False status view of
    its buffer are gone (the view's ctypes buffer holds a reference to this object)."""

    def __init__(self, h):
        self.h = h

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            try:
                lib().kv_free_result(h)
            except Exception:
                pass
            self.h = None


class Result:
    """kv_result: statuses [rule][res] (a copy, or with copy=False a read-only view of the library's
    page-locked buffer; the view keeps the result's buffers alive), per-rule counts, failing
    paths / messages."""

    def __init__(self, h, policyset: PolicySet, batch: Batch, copy: bool = True):
        self._owner = _ResultHandle(h)
        self._h = h
        self.policyset = policyset
        self.batch = batch
        L = lib()
        nr, nn = ctypes.c_uint64(), ctypes.c_uint64()
        L.kv_result_status(h, None, ctypes.byref(nr), ctypes.byref(nn))
        self.n_rules, self.n_res = nr.value, nn.value
        self._copy = copy
        self._status = None
        self._status_read = False
        c = ctypes.c_void_p()
        L.kv_result_counts(h, ctypes.byref(c))
        cb = (ctypes.c_int64 * (self.n_rules * 8)).from_address(c.value) if self.n_rules else []
        self.counts = np.frombuffer(cb, dtype=np.int64).reshape(self.n_rules, 8).copy() if self.n_rules else \
            np.zeros((0, 8), np.int64)
        self.kernel_ms = L.kv_result_kernel_ms(h)
        # wall-clock phases of the kv_validate behind this result (upload, setup, pass, fetch steps)
        self.phases = {}
        nm, ms, i = ctypes.c_char_p(), ctypes.c_double(), 0
        while L.kv_result_phase(h, i, ctypes.byref(nm), ctypes.byref(ms)) == 0:
            key = nm.value.decode()
            self.phases[key] = self.phases.get(key, 0.0) + ms.value
            i += 1
        sc, ns = ctypes.c_void_p(), ctypes.c_uint32()
        self.scope_counts = None  # [scope][rule][8] with MODE_SCOPES
        if L.kv_result_scope_counts(h, ctypes.byref(sc), ctypes.byref(ns)) == 0 and self.n_rules and ns.value:
            buf = (ctypes.c_int64 * (ns.value * self.n_rules * 8)).from_address(sc.value)
            self.scope_counts = np.frombuffer(buf, dtype=np.int64).reshape(ns.value, self.n_rules, 8).copy()

    @property
    def status(self):
        """uint8 [rule][res] statuses in the caller's order, or None for a counts-only result. The
        library materialises the matrix on first use from the form the statuses crossed PCIe in
        (kv_result_status; the segments a specialized pass wrote, 4 bits a status)."""
        if not self._status_read:
            p = ctypes.c_void_p()
            if lib().kv_result_status(self._h, ctypes.byref(p), None, None) != 0:
                raise MemoryError("kv_result_status: no host memory for the status matrix")
            if p.value:
                buf = (ctypes.c_uint8 * (self.n_rules * self.n_res)).from_address(p.value)
                buf._kv_owner = self._owner  # the view outlives this Result only together with the handle
                st = np.frombuffer(buf, dtype=np.uint8).reshape(self.n_rules, self.n_res)
                if self._copy:
                    st = st.copy()
                else:
                    st.flags.writeable = False
                self._status = st
            self._status_read = True
        return self._status

    def _text(self, fn, rule: int, res: int, *extra, errors: str = "strict", empty_ok: bool = False) -> str | None:
        """A text accessor ``fn(handle, rule, res, [extra...], buf, cap)`` of the library: its text
        (the buffer regrown while the returned length does not fit), None for a negative return
        and, unless the empty string is an answer of its own (``empty_ok``), for 0."""
        cap = 256
        while True:
            buf = ctypes.create_string_buffer(cap)
            n = fn(self._h, rule, res, *extra, buf, cap)
            if n < 0 or (n == 0 and not empty_ok):
                return None
            if n < cap:
                return buf.raw[:n].decode("utf-8", errors)
            cap = n + 1

    def path(self, rule: int, res: int) -> str | None:
        return self._text(lib().kv_result_path, rule, res, empty_ok=True)

    def precond_message(self, rule: int, res: int) -> str | None:
        """"preconditions not met" for a SKIP pair decided by the rule's preconditions
        (``kv_result_precond_message``), else None (a conditional-anchor SKIP of the pattern)."""
        return self._text(lib().kv_result_precond_message, rule, res)

    def deny_message(self, rule: int, res: int) -> str | None:
        """"failed to substitute variables in deny conditions: ..." for an ERROR pair of a device
        deny rule (``kv_result_deny_message``), else None."""
        return self._text(lib().kv_result_deny_message, rule, res)

    def foreach_element(self, rule: int, res: int) -> int | None:
        """The index in its list of the element that decided a FAIL / ERROR pair of a device foreach
        rule (``kv_result_foreach_element``), else None."""
        i = ctypes.c_uint32()
        rc = lib().kv_result_foreach_element(self._h, rule, res, ctypes.byref(i))
        return i.value if rc == 0 and i.value != 0xFFFFFFFF else None

    def foreach_entry(self, rule: int, res: int) -> int | None:
        """The position among the rule's entries of the one that decided a FAIL / ERROR pair of a
        device foreach rule (``kv_result_foreach_entry``; 0 for a rule of one entry), else None."""
        i = ctypes.c_uint32()
        rc = lib().kv_result_foreach_entry(self._h, rule, res, ctypes.byref(i))
        return i.value if rc == 0 and i.value != 0xFFFFFFFF else None

    def foreach_message(self, rule: int, res: int) -> str | None:
        """"validation failed in foreach rule for failed to substitute ..." for an ERROR pair of a
        device foreach rule, "rule skipped" for a SKIP the fold decided
        (``kv_result_foreach_message``), else None."""
        return self._text(lib().kv_result_foreach_message, rule, res)

    def foreach_path(self, rule: int, res: int) -> str | None:
        """The failing path of a FAIL pair of a device foreach rule with a pattern entry, relative to
        the deciding element (``kv_result_foreach_path``), else None."""
        return self._text(lib().kv_result_foreach_path, rule, res, empty_ok=True)

    def foreach_error_message(self, rule: int, res: int, element) -> str | None:
        """err.Error() of the pattern error of the deciding element of a FAIL / ERROR pair of a device
        foreach rule with a pattern entry (``kv_result_foreach_error_message``), else None.
        ``element`` is the caller's document of that element (dict or JSON text); its numbers are
        formatted as float64, as the reference's element is typed."""
        doc = element if isinstance(element, (bytes, str)) else _dumps(element)
        if isinstance(doc, str):
            doc = doc.encode("utf-8")
        return self._text(lib().kv_result_foreach_error_message, rule, res, doc, len(doc), errors="replace",
                          empty_ok=True)

    def foreach_alt(self, rule: int, res: int, alt: int) -> tuple[int, str | None] | None:
        """Alternative ``alt`` of the anyPattern entry that decided a FAIL pair of a device foreach
        rule, on the deciding element (``kv_result_foreach_alt``): (its status FAIL / ERROR / SKIP,
        the failing path relative to the element for FAIL, else None); None for any other pair."""
        st = ctypes.c_uint32()
        cap = 256
        while True:
            buf = ctypes.create_string_buffer(cap)
            n = lib().kv_result_foreach_alt(self._h, rule, res, alt, ctypes.byref(st), buf, cap)
            if n < 0:
                return None
            if n < cap:
                return st.value, (buf.raw[:n].decode("utf-8") if st.value == FAIL else None)
            cap = n + 1

    def foreach_alt_error_message(self, rule: int, res: int, alt: int, element) -> str | None:
        """err.Error() of the PatternError of alternative ``alt`` (``foreach_alt``) on the deciding
        element (``kv_result_foreach_alt_error_message``), else None. ``element`` as for
        ``foreach_error_message``."""
        doc = element if isinstance(element, (bytes, str)) else _dumps(element)
        if isinstance(doc, str):
            doc = doc.encode("utf-8")
        return self._text(lambda h, ru, re_, *a: lib().kv_result_foreach_alt_error_message(h, ru, re_, alt, *a), rule, res,
                          doc, len(doc), errors="replace", empty_ok=True)

    def foreach_subst_error(self, rule: int, res: int) -> str | None:
        """The RuleResponse message of an ERROR pair of a device foreach rule whose deciding element
        failed the substitution of its entry's pattern (``foreach_patvars=True``): "validation failed
        in foreach rule for variable substitution failed: ..." (``kv_result_foreach_subst_error``),
        else None."""
        return self._text(lib().kv_result_foreach_subst_error, rule, res, errors="replace")

    def subst_error(self, rule: int, res: int) -> str | None:
        """The RuleResponse message of an ERROR pair caused by the pattern's variables failing to
        substitute ("variable substitution failed: ...", ``kv_result_subst_error``), else None."""
        return self._text(lib().kv_result_subst_error, rule, res, errors="replace")

    def error_message(self, rule: int, res: int, resource) -> str | None:
        """err.Error() of the pattern error behind a FAIL / ERROR / SKIP pair (``kv_result_error_message``):
        the SKIP message, and the operand of the ERROR message. ``resource`` is the ingested document
        (dict or JSON text), from which the Go '%v' operands are formatted."""
        doc = resource if isinstance(resource, (bytes, str)) else _dumps(resource)
        if isinstance(doc, str):
            doc = doc.encode("utf-8")
        return self._text(lib().kv_result_error_message, rule, res, doc, len(doc), errors="replace", empty_ok=True)

    def failures(self):
        """Every FAIL / ERROR / SKIP pair (``kv_result_failures``), rule-major in resource order:
        (rule u32[n], res u64[n], path_id u32[n]) and ``paths`` (path_id -> string; FAIL only)."""
        n = ctypes.c_uint64()
        pr, pq, pp = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        rc = lib().kv_result_failures(self._h, ctypes.byref(n), ctypes.byref(pr), ctypes.byref(pq), ctypes.byref(pp))
        if rc != 0:
            raise _native.KvError(rc, "kv_result_failures failed")
        k = n.value
        if k == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint32), []
        rule = np.frombuffer((ctypes.c_uint32 * k).from_address(pr.value), np.uint32).copy()
        res = np.frombuffer((ctypes.c_uint64 * k).from_address(pq.value), np.uint64).copy()
        pid = np.frombuffer((ctypes.c_uint32 * k).from_address(pp.value), np.uint32).copy()
        paths = []
        while True:
            p = lib().kv_path_string(self._h, len(paths))
            if p is None:
                break
            paths.append(p.decode("utf-8"))
        return rule, res, pid, paths

    def error(self, rule: int, res: int):
        k, f = ctypes.c_uint32(), ctypes.c_uint32()
        if lib().kv_result_error(self._h, rule, res, ctypes.byref(k), ctypes.byref(f)) != 0:
            return None
        return k.value, f.value



def validate(policyset: PolicySet, batch: Batch, admission: dict | None = None,
             exclude_group_role: list | None = None, device: int = 0,
             mode: int = MODE_STATUS | MODE_ERRORS, device_mask: int | None = None, copy: bool = True) -> Result:
    """kv_validate on `device`, or kv_validate_devices over the devices of `device_mask`
    (contiguous resource shards, counts all-reduced over RCCL inside the library). copy=False: the
    status matrix is a view of the result's buffer (no host copy)."""
    ctx = {}
    if admission:
        ctx["admission"] = admission
    if exclude_group_role:
        ctx["excludeGroupRole"] = list(exclude_group_role)
    h = ctypes.c_void_p()
    err = new_err()
    if device_mask is None:
        rc = lib().kv_validate(policyset._h, batch._h, _dumps(ctx), device, mode, ctypes.byref(h), ctypes.byref(err))
    else:
        rc = lib().kv_validate_devices(policyset._h, batch._h, _dumps(ctx), device_mask, mode, ctypes.byref(h),
                                       ctypes.byref(err))
    check(rc, err)
    return Result(h, policyset, batch, copy=copy)


def bench(policyset: PolicySet, batch: Batch, device: int = 0, mode: int = MODE_COUNTS, warmup: int = 2,
          iters: int = 10, ctx: dict | None = None) -> float:
    ms = ctypes.c_double()
    err = new_err()
    check(lib().kv_bench(policyset._h, batch._h, _dumps(ctx or {}), device, mode, warmup, iters, ctypes.byref(ms),
                         ctypes.byref(err)), err)
    return ms.value


class Session:
    """Device-resident launch configuration: inputs and output buffers allocated once."""

    def __init__(self, policyset: PolicySet, batch: Batch | None, device: int = 0, mode: int = MODE_COUNTS,
                 ctx: dict | None = None, device_mask: int | None = None, parts: int = 0):
        h = ctypes.c_void_p()
        err = new_err()
        if parts:  # parts session: attach_part() uploads each part's own batch
            rc = lib().kv_session_create_parts(policyset._h, _dumps(ctx or {}), mode, parts, ctypes.byref(h),
                                               ctypes.byref(err))
        elif device_mask is None:
            rc = lib().kv_session_create(policyset._h, batch._h, _dumps(ctx or {}), device, mode, ctypes.byref(h),
                                         ctypes.byref(err))
        else:
            rc = lib().kv_session_create_devices(policyset._h, batch._h, _dumps(ctx or {}), device_mask, mode,
                                                 ctypes.byref(h), ctypes.byref(err))
        check(rc, err)
        self._h = h
        self.policyset, self.batch = policyset, batch
        self.n_rules = policyset.n_rules
        n = ctypes.c_uint32()
        lib().kv_session_parts(h, ctypes.byref(n))
        self.n_parts = n.value

    @classmethod
    def parts(cls, policyset: PolicySet, n_parts: int, mode: int = MODE_COUNTS, ctx: dict | None = None) -> "Session":
        """Multi-device session assembled from per-device batches (kv_session_create_parts): attach
        each part's batch with attach_part(); the batch may be dropped right after."""
        return cls(policyset, None, mode=mode, ctx=ctx, parts=n_parts)

    def attach_part(self, part: int, batch: Batch, device: int) -> None:
        err = new_err()
        check(lib().kv_session_attach_part(self._h, part, batch._h, device, ctypes.byref(err)), err)

    def scope_names(self) -> list[str]:
        """Scope table: the batch's namespaces, or the sorted union of the parts' namespaces."""
        n = ctypes.c_uint32()
        if lib().kv_session_scopes(self._h, ctypes.byref(n)) != 0:
            raise _native.KvError(-1, "kv_session_scopes failed (a part is not attached)")
        return [lib().kv_session_scope_name(self._h, i).decode() for i in range(n.value)]

    def rccl_ranks(self) -> int:
        """Ranks of the session's RCCL communicator (0: counts summed on the host)."""
        n = ctypes.c_int32()
        if lib().kv_session_rccl_ranks(self._h, ctypes.byref(n)) != 0:
            raise _native.KvError(-3, "kv_session_rccl_ranks failed")
        return n.value

    def status_bytes(self) -> int:
        """Status-matrix bytes the last run()'s pass wrote (unwritten segments are all NOMATCH)."""
        n = ctypes.c_uint64()
        if lib().kv_session_status_bytes(self._h, ctypes.byref(n)) != 0:
            raise _native.KvError(-3, "kv_session_status_bytes failed")
        return n.value

    def part_ms(self) -> list[float]:
        """HIP-event milliseconds of each part's last run()."""
        out = np.zeros(self.n_parts, dtype=np.float64)
        lib().kv_session_part_ms(self._h, out.ctypes.data)
        return out.tolist()

    def fetch(self) -> "Result":
        """The last pass as a result (statuses, compacted error records, reduced counts)."""
        h = ctypes.c_void_p()
        err = new_err()
        check(lib().kv_session_fetch(self._h, ctypes.byref(h), ctypes.byref(err)), err)
        return Result(h, self.policyset, self.batch)

    def run(self, iters: int) -> float:
        """Enqueue `iters` passes and wait; returns total HIP-event milliseconds."""
        ms = ctypes.c_double()
        err = new_err()
        check(lib().kv_session_run(self._h, iters, ctypes.byref(ms), ctypes.byref(err)), err)
        return ms.value

    def counts(self) -> np.ndarray:
        out = np.zeros((self.n_rules, 8), dtype=np.int64)
        rc = lib().kv_session_counts(self._h, out.ctypes.data)
        if rc != 0:
            raise _native.KvError(rc, "kv_session_counts failed")
        return out

    def scope_counts(self, n_scopes: int) -> np.ndarray:
        """[scope][rule][8] of the last pass (MODE_SCOPES)."""
        out = np.zeros((n_scopes, self.n_rules, 8), dtype=np.int64)
        rc = lib().kv_session_scope_counts(self._h, out.ctypes.data)
        if rc != 0:
            raise _native.KvError(rc, "kv_session_scope_counts failed")
        return out

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                lib().kv_free_session(h)
            except Exception:
                pass
            self._h = None


def host_reserve(nbytes: int) -> bool:
    """Page-lock `nbytes` of host memory for the library's store and result arrays once, before the
    first batch (kv_host_reserve); False without a device."""
    return lib().kv_host_reserve(int(nbytes)) == 0


def synth(seed: int, n: int, kind_mix: int = 0, first: int = 0) -> bytes:
    """NDJSON of resources [first, first + n) of the synthetic stream `seed` (kv_synth_range)."""
    p = ctypes.c_void_p()
    ln = ctypes.c_size_t()
    rc = lib().kv_synth_range(seed, first, n, kind_mix, ctypes.byref(p), ctypes.byref(ln))
    if rc != 0:
        raise _native.KvError(rc, "kv_synth failed")
    # ctypes.string_at takes a C int size: copy buffers over 2 GiB in pieces
    step = 1 << 30
    data = b"".join(ctypes.string_at(p.value + o, min(step, ln.value - o)) for o in range(0, ln.value, step)) \
        if ln.value > step else ctypes.string_at(p.value, ln.value)
    lib().kv_free_buffer(p)
    return data
