"""Reference for the preemption dry run (spec/semantics.md S18): an independent restatement in Python
integers of the pod registry, the dry run per node, the choice among candidates and qs_evict.  CPU only.

`Ref` mirrors one context: the node table (a dict of numpy columns, as qsched.Scheduler.read_nodes
returns it), the registry and the sequence counter.  `preempt(pod, variant=...)` can also answer as one
of four deliberately wrong readings of the spec (VARIANTS); tests/preempt_cases.py requires that every
parity case tells each of them from the right answer.
"""
import copy

import numpy as np

from qsched import QS_PREEMPT_BY_PRIORITY as BY_PRIORITY, QS_PREEMPT_BY_QOS as BY_QOS, VICTIM_DTYPE


VARIANTS = ("no_reprieve", "reprieve_low_first", "count_first", "priority_only")
ENTRY_FIELDS = ("seq", "priority", "qos", "app", "req_cpu", "req_mem", "req_ext", "nz_cpu", "nz_mem")


def importance(policy, qos, priority):
    base = int(priority) + (1 << 31)
    return (int(qos) << 32) + base if policy == BY_QOS else base


def _entry(pod, seq):
    return dict(seq=seq, priority=int(pod["priority"]), qos=int(pod["qos"]), app=int(pod["app"]),
                req_cpu=int(pod["req_cpu"]), req_mem=int(pod["req_mem"]),
                req_ext=(int(pod["req_ext"][0]), int(pod["req_ext"][1])),
                nz_cpu=int(pod["nz_cpu"]), nz_mem=int(pod["nz_mem"]))


def _same_pod(e, pod):
    return all(e[f] == _entry(pod, e["seq"])[f] for f in ENTRY_FIELDS)


def qos_order(pods, qos_sort=True):
    """Decision order of a stream (spec S8): stable by (qos desc, priority desc) or arrival order."""
    idx = list(range(len(pods)))
    if qos_sort:
        idx.sort(key=lambda j: (-int(pods["qos"][j]), -int(pods["priority"][j])))
    return idx


class Ref:
    def __init__(self, nodes, enable_taint=True, enable_affinity=True, policy=BY_PRIORITY, on=True):
        self.t = {k: np.array(v, copy=True) for k, v in nodes.items()}
        self.n = len(self.t["alloc_cpu"])
        self.reg = [[] for _ in range(self.n)]
        self.seq = 0
        self.on = on
        self.policy = policy
        self.enable_taint, self.enable_affinity = enable_taint, enable_affinity
        self._saved = None

    # ---- registry ----
    def imp(self, e, policy=None):
        return importance(self.policy if policy is None else policy, e["qos"], e["priority"])

    def _row_add(self, i, e, sign):
        t = self.t
        t["req_cpu"][i] += sign * e["req_cpu"]
        t["req_mem"][i] += sign * e["req_mem"]
        t["req_ext"][i, 0] += sign * e["req_ext"][0]
        t["req_ext"][i, 1] += sign * e["req_ext"][1]
        t["nz_cpu"][i] += sign * e["nz_cpu"]
        t["nz_mem"][i] += sign * e["nz_mem"]
        t["pods"][i] += sign

    def reserve(self, i, pod):
        e = _entry(pod, 0)
        self._row_add(i, e, +1)
        if self.on:
            self.seq += 1
            e["seq"] = self.seq
            self.reg[i].append(e)

    def unreserve(self, i, pod):
        """False (nothing changed) when the registry is on and holds no equal entry."""
        if self.on:
            match = [e for e in self.reg[i] if _same_pod(e, pod)]
            if not match:
                return False
            self.reg[i].remove(max(match, key=lambda e: e["seq"]))
        self._row_add(i, _entry(pod, 0), -1)
        return True

    def place_stream(self, pods, placement, qos_sort=True):
        for j in qos_order(pods, qos_sort):
            if placement[j] >= 0:
                self.reserve(int(placement[j]), pods[j])

    def evict(self, i, seq):
        hit = [e for e in self.reg[i] if e["seq"] == seq]
        if not hit:
            return False
        self.reg[i].remove(hit[0])
        self._row_add(i, hit[0], -1)
        return True

    def walk(self, i, policy=None):
        """The node's entries from most to least important (UP util.MoreImportantPod)."""
        return sorted(self.reg[i], key=lambda e: (-self.imp(e, policy), e["seq"]))

    def node_pods(self, i):
        return self.walk(i)

    def load(self, nodes):
        self.__init__(nodes, self.enable_taint, self.enable_affinity, self.policy, self.on)

    def save(self):
        self._saved = (copy.deepcopy(self.t), copy.deepcopy(self.reg), self.seq)

    def restore(self):
        t, reg, seq = self._saved
        self.t, self.reg, self.seq = copy.deepcopy(t), copy.deepcopy(reg), seq

    # ---- dry run ----
    def resolvable(self, i, pod):
        t = self.t
        if self.enable_taint and int(t["taint_hard"][i]) & ~int(pod["tol_hard"]) & ((1 << 64) - 1):
            return False
        if self.enable_affinity:
            lb = (int(t["label_bits"][i, 0]), int(t["label_bits"][i, 1]))

            def subset(m):
                return (int(m[0]) & ~lb[0]) == 0 and (int(m[1]) & ~lb[1]) == 0
            if not subset(pod["sel"]):
                return False
            nt = int(pod["n_req_terms"])
            if nt and not any(subset(pod["req_terms"][k]) for k in range(nt)):
                return False
        return True

    def _fits(self, i, pod, removed):
        """NodeResourcesFit (spec S4) on row i with the entries of `removed` taken out."""
        t = self.t
        if int(t["pods"][i]) - len(removed) + 1 > int(t["max_pods"][i]):
            return False
        for req, alloc, used, out in (
                (int(pod["req_cpu"]), int(t["alloc_cpu"][i]), int(t["req_cpu"][i]), sum(e["req_cpu"] for e in removed)),
                (int(pod["req_mem"]), int(t["alloc_mem"][i]), int(t["req_mem"][i]), sum(e["req_mem"] for e in removed)),
                (int(pod["req_ext"][0]), int(t["alloc_ext"][i, 0]), int(t["req_ext"][i, 0]),
                 sum(e["req_ext"][0] for e in removed)),
                (int(pod["req_ext"][1]), int(t["alloc_ext"][i, 1]), int(t["req_ext"][i, 1]),
                 sum(e["req_ext"][1] for e in removed))):
            if req > 0 and req > alloc - (used - out):
                return False
        return True

    def dry_run_node(self, i, pod, variant=None):
        """None (no candidate) or the victims of node i in walk order."""
        pol = BY_PRIORITY if variant == "priority_only" else self.policy
        P = importance(pol, pod["qos"], pod["priority"])
        if not self.resolvable(i, pod):
            return None
        lower = [e for e in self.walk(i, pol) if self.imp(e, pol) < P]
        if not lower:
            return None
        if not self._fits(i, pod, lower):
            return None
        if variant == "no_reprieve":
            return lower
        order = lower[::-1] if variant == "reprieve_low_first" else lower
        removed = list(lower)
        victims = []
        for e in order:
            removed.remove(e)
            if not self._fits(i, pod, removed):
                removed.append(e)
                victims.append(e)
        return victims

    def preempt(self, pod, variant=None):
        """(node, victims, nvict_n): the chosen node or -1, its victims in walk order, victims per node."""
        pol = BY_PRIORITY if variant == "priority_only" else self.policy
        nvict_n = np.full(self.n, -1, np.int32)
        best, best_key, best_v = -1, None, []
        for i in range(self.n):
            v = self.dry_run_node(i, pod, variant)
            if v is None:
                continue
            nvict_n[i] = len(v)
            if not v:
                key = (0, 0, 0, 0, 0, i)
            else:
                imps = [self.imp(e, pol) for e in v]
                hi = max(imps)
                start = min(e["seq"] for e, m in zip(v, imps) if m == hi)
                if variant == "count_first":
                    key = (1, len(v), hi, sum(imps), -start, i)
                else:
                    key = (1, hi, sum(imps), len(v), -start, i)
            if best_key is None or key < best_key:
                best, best_key, best_v = i, key, v
        return best, best_v, nvict_n


def victims_equal(got, want):
    """A VICTIM_DTYPE array from the library against the reference's entries, every field, in order."""
    assert got.dtype == VICTIM_DTYPE
    if len(got) != len(want):
        return False
    for g, e in zip(got, want):
        if (int(g["seq"]), int(g["priority"]), int(g["qos"]), int(g["app"]), int(g["req_cpu"]), int(g["req_mem"]),
                int(g["req_ext"][0]), int(g["req_ext"][1]), int(g["nz_cpu"]), int(g["nz_mem"])) != (
                e["seq"], e["priority"], e["qos"], e["app"], e["req_cpu"], e["req_mem"], e["req_ext"][0],
                e["req_ext"][1], e["nz_cpu"], e["nz_mem"]):
            return False
    return True
