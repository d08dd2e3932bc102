"""Client façade — host-side mirror of gochugaru's check family, answered locally.

Mirrors ``client/client.go``:

* ``Check``      (``:238-284``)  — items in request order; HAS_PERMISSION -> True, NO and
  CONDITIONAL -> False (``:274-277``); the first per-item error returns the results so far
  plus the error (``:279-280``); an empty request returns ``[]`` (``client_test.go:203-207``).
* ``CheckOne``   (``:129-135``), ``CheckAny`` (``:138-145``), ``CheckAll`` (``:148-160``),
  ``CheckIter``  (``:164-180``, chunks of 1000 by default, stops at the first error).
* ``checkOverlap`` (``:182-191``) — raises (Go panics) when ``WithOverlapRequired`` is set and
  the context carries no overlap key.
* ``retryRetriableErrors`` (``:193-211``) — exponential backoff 50 ms -> 2 s on Unavailable
  (``GCK_E_DEVICE``, ``GCK_E_REVISION``) and DeadlineExceeded; anything else is permanent.

The round-trip to SpiceDB (``:261-266``) is replaced by ``Engine.check_bulk`` on the GPU.
Go's ``(results, err)`` return pairs are kept as Python tuples so that callers and tests read
like the reference.
"""
from __future__ import annotations

import random
import time
from typing import Iterable, Iterator, List, Optional, Tuple

from . import consistency as _cs
from . import rel as _rel
from .consistency import Background, Context, Strategy
from .engine import (CHANGE_ANY, CHANGE_GAINED, CHANGE_LOST, CONSISTENCY_AT_LEAST, CONSISTENCY_FULL, CONSISTENCY_MIN_LATENCY,
                     CONSISTENCY_SNAPSHOT, ELLIPSIS, GCK_E_DEVICE, GCK_E_NOT_FOUND, GCK_E_REVISION,
                     ID_ABSENT, ID_WILDCARD, ITEM_ERROR_MESSAGES, PERM_HAS, REL_INVALID, TYPE_INVALID,
                     VARY_RESOURCE, VARY_SUBJECT, Engine, GckError, shape_request, unpack_cross, unpack_results)

CHECK_ITER_CHUNK = 1000  # client/client.go:166


class OverlapKeyPanic(RuntimeError):
    """Go panics in checkOverlap (client/client.go:190)."""


class CheckItemError(Exception):
    """A CheckBulkPermissionsPair_Error turned into a Go error (client/client.go:279-280)."""


class Unavailable(Exception):
    pass


class InvalidArgument(Exception):
    pass


def WithOverlapRequired():
    """``client/client.go:84-86``."""
    def opt(c: "Client"):
        c.overlapRequired = True
    return opt


def WithCompactRequests():
    """Check sends every request of at most 64 shapes — (resource type, permission, subject type,
    subject relation, context slot) — as a shaped request (Engine.check_shaped: a shape table, one
    index byte and one id pair per check in, 2-bit results out) instead of 20-B items. The
    ``(results, err)`` it returns are the same."""
    def opt(c: "Client"):
        c.compactRequests = True
    return opt


def _requirement(cs: Optional[Strategy]) -> Tuple[int, int]:
    if cs is None:
        return CONSISTENCY_MIN_LATENCY, 0
    v = cs.V1Consistency
    if v.requirement == _cs.MINIMIZE_LATENCY:
        return CONSISTENCY_MIN_LATENCY, 0
    if v.requirement == _cs.FULLY_CONSISTENT:
        return CONSISTENCY_FULL, 0
    try:
        rev = int(v.token)
    except (TypeError, ValueError):
        raise InvalidArgument(f"invalid zedtoken {v.token!r}")
    if v.requirement == _cs.AT_LEAST_AS_FRESH:
        return CONSISTENCY_AT_LEAST, rev
    if v.requirement == _cs.AT_EXACT_SNAPSHOT:
        return CONSISTENCY_SNAPSHOT, rev
    raise InvalidArgument(f"unknown consistency requirement {v.requirement!r}")


def _retriable(err: BaseException) -> bool:
    if isinstance(err, GckError):
        return err.code in (GCK_E_DEVICE, GCK_E_REVISION)  # gRPC Unavailable
    msg = str(err)
    return isinstance(err, (Unavailable, TimeoutError)) or \
        "retryable error" in msg or "try restarting transaction" in msg


def retryRetriableErrors(ctx: Context, fn, max_elapsed: float = 15 * 60):
    """``client/client.go:193-211``: backoff.ExponentialBackOff{Initial 50ms, Max 2s,
    default multiplier 1.5 and randomization 0.5}; gives up at the context deadline (or the
    backoff's default 15 min max elapsed time)."""
    interval = 0.05
    start = time.monotonic()
    deadline = getattr(ctx, "deadline", None)
    while True:
        try:
            return fn()
        except Exception as err:  # noqa: BLE001 — classified below
            if not _retriable(err):
                raise
            delay = interval * (1 + random.uniform(-0.5, 0.5))
            now = time.monotonic()
            limit = start + max_elapsed if deadline is None else deadline
            if now + delay > limit:
                raise
            time.sleep(delay)
            interval = min(interval * 1.5, 2.0)


class Client:
    """``client.Client`` (``client/client.go:101-105``) with a local GPU evaluator in place of
    the gRPC connection."""

    def __init__(self, engine: Engine, *opts, chunk: int = 65536):
        self.engine = engine
        self.overlapRequired = False
        self.compactRequests = False
        self.chunk = chunk
        for o in opts:
            o(self)

    @classmethod
    def NewWithOpts(cls, engine: Engine, *opts) -> Tuple["Client", Optional[Exception]]:
        """``client/client.go:65-75``."""
        return cls(engine, *opts), None

    # ---- overlap guard -------------------------------------------------------------------
    def checkOverlap(self, ctx: Optional[Context]):
        if self.overlapRequired:
            md = (ctx or Background).metadata
            if md.get(_cs.REQUEST_OVERLAP_KEY):
                return
            raise OverlapKeyPanic("failed to configure required overlap key for request")

    # ---- the check family ----------------------------------------------------------------
    def Check(self, ctx: Optional[Context], cs: Optional[Strategy], *rs) -> Tuple[List[bool], Optional[Exception]]:
        self.checkOverlap(ctx)
        rels = [r.Relationship() for r in rs]
        try:
            requirement, revision = _requirement(cs)

            def attempt():
                # interned per attempt, like the server resolving names at evaluation time: an
                # object a Watch batch created while this request waited is found on the retry
                items, contexts = self.engine.make_request(rels)
                shaped = shape_request(items) if self.compactRequests and len(items) else None
                if shaped is None:
                    return self.engine.check_bulk(items, requirement, revision, contexts=contexts)
                words, errs, _ = self.engine.check_shaped(*shaped, requirement, revision, contexts=contexts)
                return unpack_results(words, len(items)), errs
            perm, err = retryRetriableErrors(ctx or Background, attempt)
            if err.dtype.names:  # a shaped request's error list: ascending (index, code) records
                first = err[0] if len(err) else None
                n_ok = int(first["index"]) if first is not None else len(perm)
                results = [p == PERM_HAS for p in perm[:n_ok].tolist()]
                if first is None:
                    return results, None
                e = int(first["code"])
                return results, CheckItemError(ITEM_ERROR_MESSAGES.get(e, f"item error {e}"))
        except Exception as e:  # noqa: BLE001 — Go returns (nil, err)
            return None, e
        results: List[bool] = []
        for p, e in zip(perm.tolist(), err.tolist()):
            if e:
                return results, CheckItemError(ITEM_ERROR_MESSAGES.get(e, f"item error {e}"))
            results.append(p == PERM_HAS)
        return results, None

    def CheckCross(self, ctx: Optional[Context], cs: Optional[Strategy], permission: str, resources: Iterable[str],
                   subjects: Iterable[str]) -> Tuple[Optional[List[List[bool]]], Optional[Exception]]:
        """Every subject against every resource under one permission, as one cross request
        (Engine.check_cross: the two id lists in, 2-bit results out) — what ``Check`` answers for
        the len(subjects) x len(resources) relationships ``resource#permission@subject``, without
        building them. ``resources`` are object strings of one type ("document:readme"), ``subjects``
        of one kind ("user:jimmy", or all "group:eng#member"); mixed types are InvalidArgument.
        Returns ``(rows, err)``: rows[s][r] is True iff subject s HAS the permission on resource r
        (NO and CONDITIONAL are False, an unknown name is a nonexistent object). The first per-item
        error, in row-major order, returns the rows up to it and a CheckItemError, as ``Check``."""
        self.checkOverlap(ctx)
        try:
            res = [_rel.ParseObjectSet(r) for r in resources]
            sub = [_rel.ParseObjectSet(s) for s in subjects]
            if len({t for t, _, _ in res}) > 1 or any(rel for _, _, rel in res):
                raise InvalidArgument("CheckCross: the resources must be objects of one type")
            if len({(t, rel if rel not in ("", "...") else "") for t, _, rel in sub}) > 1:
                raise InvalidArgument("CheckCross: the subjects must be of one type and relation")
            if not res or not sub:
                return [[] for _ in sub], None
            requirement, revision = _requirement(cs)
            eng = self.engine
            S, R = len(sub), len(res)

            def attempt():
                # interned per attempt, as Check does
                rt, st = eng.type_id(res[0][0]), eng.type_id(sub[0][0])
                srel = ELLIPSIS if sub[0][2] in ("", "...") else eng.relation_id(st, sub[0][2])
                rids = eng.intern(rt, [i for _, i, _ in res]) if rt != TYPE_INVALID else [ID_ABSENT] * R
                if st != TYPE_INVALID:
                    sids = eng.intern(st, [i for _, i, _ in sub])
                else:
                    sids = [ID_WILDCARD if i == "*" else ID_ABSENT for _, i, _ in sub]
                header = (rt, eng.relation_id(rt, permission), st, srel)
                words, errs, _ = eng.check_cross(header, sids, rids, requirement, revision)
                return unpack_cross(words, S, R), errs
            perm, errs = retryRetriableErrors(ctx or Background, attempt)
            has = (perm == PERM_HAS)
            if not len(errs):
                return has.tolist(), None
            at, e = int(errs[0]["index"]), int(errs[0]["code"])
            rows = has[:at // R].tolist()
            rows.append(has[at // R, :at % R].tolist())
            return rows, CheckItemError(ITEM_ERROR_MESSAGES.get(e, f"item error {e}"))
        except Exception as e:  # noqa: BLE001 — Go returns (nil, err)
            return None, e

    def CheckOne(self, ctx, cs, r) -> Tuple[bool, Optional[Exception]]:
        results, err = self.Check(ctx, cs, r)
        if err is not None:
            return False, err
        return results[0], None

    def CheckAny(self, ctx, cs, *rs) -> Tuple[bool, Optional[Exception]]:
        results, err = self.Check(ctx, cs, *rs)
        if err is not None:
            return False, err
        return True in results, None

    def CheckAll(self, ctx, cs, *rs) -> Tuple[bool, Optional[Exception]]:
        results, err = self.Check(ctx, cs, *rs)
        if err is not None:
            return False, err
        for r in results:
            if not r:
                return False, None
        return True, None

    def CheckIter(self, ctx, cs, rs: Iterable, chunk: int = CHECK_ITER_CHUNK) -> Iterator[Tuple[bool, Optional[Exception]]]:
        buf = []
        for r in rs:
            buf.append(r)
            if len(buf) == chunk:
                ok = yield from self._iter_chunk(ctx, cs, buf)
                if not ok:
                    return
                buf = []
        if buf:
            yield from self._iter_chunk(ctx, cs, buf)

    def _iter_chunk(self, ctx, cs, items):
        checks, err = self.Check(ctx, cs, *items)
        if err is not None:
            yield False, err
            return False
        for c in checks:
            yield c, None
        return True

    # ---- lookups (client/client.go:501-599) ------------------------------------------------
    def LookupResources(self, ctx: Optional[Context], cs: Optional[Strategy], permission: str,
                        subject: str) -> Iterator[Tuple[str, Optional[Exception]]]:
        """``client/client.go:508-552``: yields the ids of the objects of ``permission``'s type
        ("document#reader") on which ``subject`` ("user:jimmy" or "team:admin#member") has the
        permission (HAS or CONDITIONAL, as SpiceDB streams both); stops at the first error."""
        self.checkOverlap(ctx)
        try:
            subj_type, subj_id, subj_rel = _rel.ParseObjectSet(subject)
            obj_type, obj_rel = _rel.ParseTypedRelation(permission)
            requirement, revision = _requirement(cs)
            eng = self.engine
            rt = eng.type_id(obj_type)
            st = eng.type_id(subj_type)
            perm = eng.relation_id(rt, obj_rel)
            srel = ELLIPSIS if subj_rel in ("", "...") else eng.relation_id(st, subj_rel)
            if TYPE_INVALID in (rt, st) or REL_INVALID in (perm, srel):
                raise GckError(GCK_E_NOT_FOUND, "object definition or relation not found")
            sid = int(eng.intern(st, [subj_id])[0])  # unknown ids stay ABSENT: wildcards still match
            ids, _ = retryRetriableErrors(ctx or Background, lambda: eng.lookup_resources(
                rt, perm, st, srel, sid, requirement, revision))
            names = [eng.object_name(rt, int(i)) for i in ids]
        except Exception as e:  # noqa: BLE001 — Go yields ("", err) and stops
            yield "", e
            return
        for n in names:
            yield n, None

    def LookupSubjects(self, ctx: Optional[Context], cs: Optional[Strategy], resource: str, permission: str,
                       subject: str) -> Iterator[Tuple[str, Optional[Exception]]]:
        """``client/client.go:560-599``: yields the ids of the subjects of type ``subject``
        ("user" or "team#member") that have ``permission`` on ``resource`` ("document:README");
        a wildcard grant yields "*" once (as SpiceDB streams it), not every subject of the type."""
        self.checkOverlap(ctx)
        try:
            res_type, res_id, _ = _rel.ParseObjectSet(resource)
            subj_type, subj_rel, _ = _rel._cut(subject, "#")
            requirement, revision = _requirement(cs)
            eng = self.engine
            rt = eng.type_id(res_type)
            st = eng.type_id(subj_type)
            perm = eng.relation_id(rt, permission)
            srel = ELLIPSIS if subj_rel in ("", "...") else eng.relation_id(st, subj_rel)
            if TYPE_INVALID in (rt, st) or REL_INVALID in (perm, srel):
                raise GckError(GCK_E_NOT_FOUND, "object definition or relation not found")
            rid = int(eng.intern(rt, [res_id])[0])
            ids, _ = retryRetriableErrors(ctx or Background, lambda: eng.lookup_subjects(
                rt, rid, perm, st, srel, requirement, revision)) if rid != ID_ABSENT else ([], [])
            # a wildcard grant is the subject "*" (SpiceDB's LookupSubjects result for `type:*`)
            names = ["*" if int(i) == ID_WILDCARD else eng.object_name(st, int(i)) for i in ids]
        except Exception as e:  # noqa: BLE001
            yield "", e
            return
        for n in names:
            yield n, None

    # ---- lookups among the caller's candidates (Engine.lookup_*_among: one list request) ------
    def _filter(self, ctx, cs, what, candidates, among):
        """FilterResources / FilterSubjects after their own parsing: `candidates` are (name, kind)
        with one kind; among(ids) runs the lookup on the candidates' ids (interned per attempt, as
        CheckCross does) and returns the matching ids. Yields the matching names in the caller's
        order, repeats included."""
        try:
            if len({k for _, k in candidates}) > 1:
                raise InvalidArgument(f"{what}: the candidates must be of one type and relation")
            if not candidates:
                return
            names = [n for n, _ in candidates]
            cand, got = retryRetriableErrors(ctx or Background, lambda: among(names))
            # (the answer is the matching candidates in order: a candidate matches iff its id is among them;
            # an unknown name is ID_ABSENT, which matches when a wildcard grants the permission)
            hit = set(int(i) for i in got)
            out = [n for n, i in zip(names, cand) if int(i) in hit]
        except Exception as e:  # noqa: BLE001 — Go yields ("", err) and stops
            yield "", e
            return
        for n in out:
            yield n, None

    def FilterResources(self, ctx: Optional[Context], cs: Optional[Strategy], permission: str, subject: str,
                        resources: Iterable[str]) -> Iterator[Tuple[str, Optional[Exception]]]:
        """Of ``resources`` — object strings of ``permission``'s type ("document#view", the form
        ``LookupResources`` takes; "document:readme") — yields the ids of those on which ``subject``
        has the permission (HAS or CONDITIONAL, as ``LookupResources``), in the caller's order and as
        often as the caller names them; stops at the first error. One list request of 4 B per
        candidate (Engine.lookup_resources_among) instead of a sweep of the whole type. An unknown
        name is a nonexistent object; resources of another type are InvalidArgument."""
        self.checkOverlap(ctx)
        try:
            subj_type, subj_id, subj_rel = _rel.ParseObjectSet(subject)
            obj_type, obj_rel = _rel.ParseTypedRelation(permission)
            res = [_rel.ParseObjectSet(r) for r in resources]
            if any(t != obj_type or rel for t, _, rel in res):
                raise InvalidArgument("FilterResources: the resources must be objects of the permission's type")
            requirement, revision = _requirement(cs)
            eng = self.engine

            def among(names):
                rt, st = eng.type_id(obj_type), eng.type_id(subj_type)
                perm = eng.relation_id(rt, obj_rel)
                srel = ELLIPSIS if subj_rel in ("", "...") else eng.relation_id(st, subj_rel)
                if TYPE_INVALID in (rt, st) or REL_INVALID in (perm, srel):
                    raise GckError(GCK_E_NOT_FOUND, "object definition or relation not found")
                sid = int(eng.intern(st, [subj_id])[0])
                cand = eng.intern(rt, names)
                return cand, eng.lookup_resources_among(rt, perm, st, srel, sid, cand, requirement, revision)[0]
        except Exception as e:  # noqa: BLE001
            yield "", e
            return
        yield from self._filter(ctx, cs, "FilterResources", [(i, t) for t, i, _ in res], among)

    def FilterSubjects(self, ctx: Optional[Context], cs: Optional[Strategy], resource: str, permission: str,
                       subjects: Iterable[str]) -> Iterator[Tuple[str, Optional[Exception]]]:
        """The mirror: of ``subjects`` — of one type and relation ("user:jimmy", or all
        "team:eng#member") — yields the ids of those that have ``permission`` on ``resource``
        ("document:readme"), in the caller's order. A wildcard grant makes every candidate match;
        no "*" is yielded."""
        self.checkOverlap(ctx)
        try:
            res_type, res_id, _ = _rel.ParseObjectSet(resource)
            sub = [_rel.ParseObjectSet(s) for s in subjects]
            requirement, revision = _requirement(cs)
            eng = self.engine

            def among(names):
                stype, srel_name = sub[0][0], sub[0][2]
                rt, st = eng.type_id(res_type), eng.type_id(stype)
                perm = eng.relation_id(rt, permission)
                srel = ELLIPSIS if srel_name in ("", "...") else eng.relation_id(st, srel_name)
                if TYPE_INVALID in (rt, st) or REL_INVALID in (perm, srel):
                    raise GckError(GCK_E_NOT_FOUND, "object definition or relation not found")
                rid = int(eng.intern(rt, [res_id])[0])
                cand = eng.intern(st, names)
                return cand, eng.lookup_subjects_among(rt, rid, perm, st, cand, srel, requirement, revision)[0]
        except Exception as e:  # noqa: BLE001
            yield "", e
            return
        yield from self._filter(ctx, cs, "FilterSubjects",
                                [(i, (t, rel if rel not in ("", "...") else "")) for t, i, rel in sub], among)

    # ---- the same over candidates that live on the device (Engine.filter_ids) -----------------
    def _filter_device(self, ctx, what, candidates, run):
        """FilterResourcesDevice / FilterSubjectsDevice after their own parsing: run() resolves the
        names and filters the tensor (per attempt, as _filter does). Returns (ids, err)."""
        try:
            import torch
            if not isinstance(candidates, torch.Tensor) or candidates.dtype not in (torch.int32, torch.uint32) \
                    or not candidates.is_cuda:
                raise InvalidArgument(f"{what}: the candidates must be a device int32 / uint32 tensor of interned ids")
            if candidates.numel() == 0:
                return candidates.reshape(-1)[:0], None
            return retryRetriableErrors(ctx or Background, run), None
        except Exception as e:  # noqa: BLE001
            return None, e

    def FilterResourcesDevice(self, ctx: Optional[Context], cs: Optional[Strategy], permission: str, subject: str,
                              candidates):
        """``FilterResources`` for candidates in device memory: ``candidates`` is a device int32 /
        uint32 tensor of interned ids (``Engine.intern``) of ``permission``'s type ("document#view").
        Returns ``(tensor, err)``: the ids on which ``subject`` has the permission (HAS or
        CONDITIONAL), on the device, in the tensor's order and as often as it repeats them — checked
        and compacted by kernels (Engine.filter_ids); only two count words come back to the host."""
        self.checkOverlap(ctx)
        try:
            subj_type, subj_id, subj_rel = _rel.ParseObjectSet(subject)
            obj_type, obj_rel = _rel.ParseTypedRelation(permission)
            requirement, revision = _requirement(cs)
            eng = self.engine

            def run():
                rt, st = eng.type_id(obj_type), eng.type_id(subj_type)
                perm = eng.relation_id(rt, obj_rel)
                srel = ELLIPSIS if subj_rel in ("", "...") else eng.relation_id(st, subj_rel)
                if TYPE_INVALID in (rt, st) or REL_INVALID in (perm, srel):
                    raise GckError(GCK_E_NOT_FOUND, "object definition or relation not found")
                sid = int(eng.intern(st, [subj_id])[0])
                return eng.filter_ids((rt, perm, st, srel), sid, VARY_RESOURCE, candidates, requirement=requirement,
                                      revision=revision)
        except Exception as e:  # noqa: BLE001
            return None, e
        return self._filter_device(ctx, "FilterResourcesDevice", candidates, run)

    def FilterSubjectsDevice(self, ctx: Optional[Context], cs: Optional[Strategy], resource: str, permission: str,
                             subject_type: str, candidates):
        """The mirror: of the candidate subjects — interned ids of ``subject_type`` ("user", or
        "team#member") in a device tensor — those that have ``permission`` on ``resource``
        ("document:readme"). A wildcard grant makes every candidate match."""
        self.checkOverlap(ctx)
        try:
            res_type, res_id, _ = _rel.ParseObjectSet(resource)
            stype, srel_name, _ = _rel._cut(subject_type, "#")
            requirement, revision = _requirement(cs)
            eng = self.engine

            def run():
                rt, st = eng.type_id(res_type), eng.type_id(stype)
                perm = eng.relation_id(rt, permission)
                srel = ELLIPSIS if srel_name in ("", "...") else eng.relation_id(st, srel_name)
                if TYPE_INVALID in (rt, st) or REL_INVALID in (perm, srel):
                    raise GckError(GCK_E_NOT_FOUND, "object definition or relation not found")
                rid = int(eng.intern(rt, [res_id])[0])
                return eng.filter_ids((rt, perm, st, srel), rid, VARY_SUBJECT, candidates, requirement=requirement,
                                      revision=revision)
        except Exception as e:  # noqa: BLE001
            return None, e
        return self._filter_device(ctx, "FilterSubjectsDevice", candidates, run)

    def CheckCrossDevice(self, ctx: Optional[Context], cs: Optional[Strategy], permission: str, resources,
                         subject_type: str, subjects):
        """``CheckCross`` for id lists in device memory — a batch of users against a page of
        candidates: ``resources`` are interned ids (``Engine.intern``) of ``permission``'s type
        ("document#view"), ``subjects`` of ``subject_type`` ("user", or "team#member"), both device
        int32 / uint32 tensors. Returns ``(plane, err)``: the len(subjects) x ceil(len(resources) / 32)
        int64 device tensor of 2-bit Permissionships (``unpack_cross``'s layout; (s, r) HAS iff its
        two bits are PERM_HAS), written by the kernels where it lies (Engine.check_cross_ids); only
        the error count comes back to the host, and a per-item error is ``err`` with no plane."""
        self.checkOverlap(ctx)
        try:
            import torch
            obj_type, obj_rel = _rel.ParseTypedRelation(permission)
            stype, srel_name, _ = _rel._cut(subject_type, "#")
            for what, t in (("resources", resources), ("subjects", subjects)):
                if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.uint32) or not t.is_cuda:
                    raise InvalidArgument(f"CheckCrossDevice: the {what} must be a device int32 / uint32 tensor of "
                                          "interned ids")
            requirement, revision = _requirement(cs)
            eng = self.engine

            def run():
                # resolved per attempt, as CheckCross does
                rt, st = eng.type_id(obj_type), eng.type_id(stype)
                perm = eng.relation_id(rt, obj_rel)
                srel = ELLIPSIS if srel_name in ("", "...") else eng.relation_id(st, srel_name)
                if TYPE_INVALID in (rt, st) or REL_INVALID in (perm, srel):
                    raise GckError(GCK_E_NOT_FOUND, "object definition or relation not found")
                return eng.check_cross_ids((rt, perm, st, srel), subjects, resources, requirement=requirement,
                                           revision=revision)
            return retryRetriableErrors(ctx or Background, run), None
        except Exception as e:  # noqa: BLE001 — Go returns (nil, err)
            return None, e

    def FilterCrossDevice(self, ctx: Optional[Context], cs: Optional[Strategy], permission: str, resources,
                          subject_type: str, subjects, limit: int = 0):
        """``CheckCrossDevice`` answered as what the caller asked: for each of ``subjects``, which of
        ``resources`` it may see (HAS or CONDITIONAL) — with ``limit``, the first ``limit`` of them in
        the page's order. Returns ``((row_off, ids), err)``: ``ids[row_off[s]:row_off[s + 1]]`` are
        subject s's permitted resource ids, both device tensors, selected and compacted by kernels over
        the finished plane (Engine.filter_cross_ids); only two count words come back to the host, and
        a per-item error is ``err``. Parsing and error mapping are ``CheckCrossDevice``'s."""
        self.checkOverlap(ctx)
        try:
            import torch
            obj_type, obj_rel = _rel.ParseTypedRelation(permission)
            stype, srel_name, _ = _rel._cut(subject_type, "#")
            for what, t in (("resources", resources), ("subjects", subjects)):
                if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.uint32) or not t.is_cuda:
                    raise InvalidArgument(f"FilterCrossDevice: the {what} must be a device int32 / uint32 tensor of "
                                          "interned ids")
            if limit < 0:
                raise InvalidArgument("FilterCrossDevice: the limit must not be negative")
            requirement, revision = _requirement(cs)
            eng = self.engine

            def run():
                # resolved per attempt, as CheckCross does
                rt, st = eng.type_id(obj_type), eng.type_id(stype)
                perm = eng.relation_id(rt, obj_rel)
                srel = ELLIPSIS if srel_name in ("", "...") else eng.relation_id(st, srel_name)
                if TYPE_INVALID in (rt, st) or REL_INVALID in (perm, srel):
                    raise GckError(GCK_E_NOT_FOUND, "object definition or relation not found")
                return eng.filter_cross_ids((rt, perm, st, srel), subjects, resources, row_limit=limit,
                                            requirement=requirement, revision=revision)
            return retryRetriableErrors(ctx or Background, run), None
        except Exception as e:  # noqa: BLE001 — Go returns (nil, err)
            return None, e

    # ---- recheck requests (Engine.recheck_ids / recheck_cross_ids): what changed since the plane kept ----
    def _recheck_list(self, ctx, cs, what, fixed, names, vary, types, prev, transitions):
        """RecheckResourcesDevice / RecheckSubjectsDevice after their own parsing. types() resolves
        (header, fixed type, varying type) per attempt. Returns ((plane, revision, changes), err)."""
        try:
            import numpy as np
            import torch
            names = list(names)
            requirement, revision = _requirement(cs)
            eng = self.engine

            def run():
                hdr, fixed_type, vary_type = types()
                fid = int(eng.intern(fixed_type, [fixed])[0])
                ids = torch.from_numpy(np.ascontiguousarray(eng.intern(vary_type, names), dtype=np.uint32).view(np.int32))
                ids = ids.to(torch.device("cuda", eng.device))
                plane, rev, _, pos, trans = eng.recheck_ids(hdr, fid, vary, ids, prev=prev, transitions=transitions,
                                                            requirement=requirement, revision=revision)
                return plane, rev, [(names[p], t >> 2, t & 3) for p, t in zip(pos.tolist(), trans.tolist())]
            return retryRetriableErrors(ctx or Background, run), None
        except Exception as e:  # noqa: BLE001 — Go returns (nil, err)
            return None, e

    def RecheckResourcesDevice(self, ctx: Optional[Context], cs: Optional[Strategy], permission: str, subject: str,
                               resources: Iterable[str], prev=None, transitions: int = CHANGE_ANY):
        """Which of ``resources`` (ids of ``permission``'s type, "document#view") changed for
        ``subject`` since ``prev``, the plane an earlier call with the same arguments returned (None:
        nothing was granted, so ``CHANGE_GAINED`` yields the initial grant set). The request is
        evaluated at the strategy's revision and compared with ``prev`` on the device
        (Engine.recheck_ids); only count words and the change records come back. Returns
        ``((plane, revision, changes), err)``: the new plane (a device tensor: the next call's
        ``prev``), the evaluated revision and ``[(resource id, old, new), ...]`` in the caller's order,
        old and new the PERM_* values of the selected ``transitions`` (``CHANGE_*``)."""
        self.checkOverlap(ctx)
        try:
            subj_type, subj_id, subj_rel = _rel.ParseObjectSet(subject)
            obj_type, obj_rel = _rel.ParseTypedRelation(permission)
            eng = self.engine

            def types():
                rt, st = eng.type_id(obj_type), eng.type_id(subj_type)
                perm = eng.relation_id(rt, obj_rel)
                srel = ELLIPSIS if subj_rel in ("", "...") else eng.relation_id(st, subj_rel)
                if TYPE_INVALID in (rt, st) or REL_INVALID in (perm, srel):
                    raise GckError(GCK_E_NOT_FOUND, "object definition or relation not found")
                return (rt, perm, st, srel), st, rt
        except Exception as e:  # noqa: BLE001
            return None, e
        return self._recheck_list(ctx, cs, "RecheckResourcesDevice", subj_id, resources, VARY_RESOURCE, types, prev,
                                  transitions)

    def RecheckSubjectsDevice(self, ctx: Optional[Context], cs: Optional[Strategy], resource: str, permission: str,
                              subject_type: str, subjects: Iterable[str], prev=None, transitions: int = CHANGE_ANY):
        """The mirror: which of ``subjects`` (ids of ``subject_type``, "user" or "team#member") changed
        on ``resource`` ("document:readme") for ``permission`` since ``prev``. Returns
        ``((plane, revision, [(subject id, old, new), ...]), err)``."""
        self.checkOverlap(ctx)
        try:
            res_type, res_id, _ = _rel.ParseObjectSet(resource)
            stype, srel_name, _ = _rel._cut(subject_type, "#")
            eng = self.engine

            def types():
                rt, st = eng.type_id(res_type), eng.type_id(stype)
                perm = eng.relation_id(rt, permission)
                srel = ELLIPSIS if srel_name in ("", "...") else eng.relation_id(st, srel_name)
                if TYPE_INVALID in (rt, st) or REL_INVALID in (perm, srel):
                    raise GckError(GCK_E_NOT_FOUND, "object definition or relation not found")
                return (rt, perm, st, srel), rt, st
        except Exception as e:  # noqa: BLE001
            return None, e
        return self._recheck_list(ctx, cs, "RecheckSubjectsDevice", res_id, subjects, VARY_SUBJECT, types, prev,
                                  transitions)

    def RecheckCrossDevice(self, ctx: Optional[Context], cs: Optional[Strategy], permission: str,
                           resources: Iterable[str], subject_type: str, subjects: Iterable[str], prev=None,
                           transitions: int = CHANGE_ANY):
        """Every one of ``subjects`` (ids of ``subject_type``) against every one of ``resources`` (ids
        of ``permission``'s type), compared with ``prev``, the plane an earlier call with the same
        arguments returned (None: nothing was granted). Returns ``((plane, revision, changes), err)``:
        the new plane (a device tensor, the next call's ``prev``), the evaluated revision and
        ``[(subject id, resource id, old, new), ...]`` by subject and then in the resources' order
        (Engine.recheck_cross_ids)."""
        self.checkOverlap(ctx)
        try:
            import numpy as np
            import torch
            obj_type, obj_rel = _rel.ParseTypedRelation(permission)
            stype, srel_name, _ = _rel._cut(subject_type, "#")
            resources, subjects = list(resources), list(subjects)
            requirement, revision = _requirement(cs)
            eng = self.engine

            def run():
                rt, st = eng.type_id(obj_type), eng.type_id(stype)
                perm = eng.relation_id(rt, obj_rel)
                srel = ELLIPSIS if srel_name in ("", "...") else eng.relation_id(st, srel_name)
                if TYPE_INVALID in (rt, st) or REL_INVALID in (perm, srel):
                    raise GckError(GCK_E_NOT_FOUND, "object definition or relation not found")
                dev = torch.device("cuda", eng.device)
                up = lambda t, names: torch.from_numpy(
                    np.ascontiguousarray(eng.intern(t, names), dtype=np.uint32).view(np.int32)).to(dev)
                plane, rev, row_off, _, col, trans = eng.recheck_cross_ids(
                    (rt, perm, st, srel), up(st, subjects), up(rt, resources), prev=prev, transitions=transitions,
                    requirement=requirement, revision=revision)
                off = row_off.tolist()
                col, trans = col.tolist(), trans.tolist()
                return plane, rev, [(subjects[s], resources[col[k]], trans[k] >> 2, trans[k] & 3)
                                    for s in range(len(subjects)) for k in range(off[s], off[s + 1])]
            return retryRetriableErrors(ctx or Background, run), None
        except Exception as e:  # noqa: BLE001 — Go returns (nil, err)
            return None, e

    def FilterCrossSubjectsDevice(self, ctx: Optional[Context], cs: Optional[Strategy], resource_permission: str,
                                  resources, subject_type: str, subjects, limit: int = 0):
        """``FilterCrossDevice`` by resource — an access review, a share dialog, a notification fan-out:
        for each of ``resources``, which of ``subjects`` may see it (HAS or CONDITIONAL) — with
        ``limit``, the first ``limit`` of them in the subject list's order. Returns
        ``((col_off, ids), err)``: ``ids[col_off[r]:col_off[r + 1]]`` are the subject ids that may see
        resource r, both device tensors, selected and compacted by kernels over the finished plane
        (Engine.filter_cross_cols_ids); only two count words come back to the host, and a per-item
        error is ``err``. Parsing and error mapping are ``FilterCrossDevice``'s."""
        self.checkOverlap(ctx)
        try:
            import torch
            obj_type, obj_rel = _rel.ParseTypedRelation(resource_permission)
            stype, srel_name, _ = _rel._cut(subject_type, "#")
            for what, t in (("resources", resources), ("subjects", subjects)):
                if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.uint32) or not t.is_cuda:
                    raise InvalidArgument(f"FilterCrossSubjectsDevice: the {what} must be a device int32 / uint32 "
                                          "tensor of interned ids")
            if limit < 0:
                raise InvalidArgument("FilterCrossSubjectsDevice: the limit must not be negative")
            requirement, revision = _requirement(cs)
            eng = self.engine

            def run():
                # resolved per attempt, as CheckCross does
                rt, st = eng.type_id(obj_type), eng.type_id(stype)
                perm = eng.relation_id(rt, obj_rel)
                srel = ELLIPSIS if srel_name in ("", "...") else eng.relation_id(st, srel_name)
                if TYPE_INVALID in (rt, st) or REL_INVALID in (perm, srel):
                    raise GckError(GCK_E_NOT_FOUND, "object definition or relation not found")
                return eng.filter_cross_cols_ids((rt, perm, st, srel), subjects, resources, col_limit=limit,
                                                 requirement=requirement, revision=revision)
            return retryRetriableErrors(ctx or Background, run), None
        except Exception as e:  # noqa: BLE001 — Go returns (nil, err)
            return None, e

    def _filter_groups(self, name: str, ctx, cs, permission: str, subject_type: str, owners, offsets, candidates,
                       vary: int, limit: int):
        self.checkOverlap(ctx)
        try:
            import torch
            obj_type, obj_rel = _rel.ParseTypedRelation(permission)
            stype, srel_name, _ = _rel._cut(subject_type, "#")
            for what, t in (("owners", owners), ("offsets", offsets), ("candidates", candidates)):
                if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.uint32) or not t.is_cuda:
                    raise InvalidArgument(f"{name}: the {what} must be a device int32 / uint32 tensor")
            if limit < 0:
                raise InvalidArgument(f"{name}: the limit must not be negative")
            requirement, revision = _requirement(cs)
            eng = self.engine

            def run():
                # resolved per attempt, as CheckCross does
                rt, st = eng.type_id(obj_type), eng.type_id(stype)
                perm = eng.relation_id(rt, obj_rel)
                srel = ELLIPSIS if srel_name in ("", "...") else eng.relation_id(st, srel_name)
                if TYPE_INVALID in (rt, st) or REL_INVALID in (perm, srel):
                    raise GckError(GCK_E_NOT_FOUND, "object definition or relation not found")
                return eng.filter_groups_ids((rt, perm, st, srel), owners, offsets, candidates, vary=vary,
                                             group_limit=limit, requirement=requirement, revision=revision)
            return retryRetriableErrors(ctx or Background, run), None
        except Exception as e:  # noqa: BLE001 — Go returns (nil, err)
            return None, e

    def FilterGroupsDevice(self, ctx: Optional[Context], cs: Optional[Strategy], permission: str, candidates, offsets,
                           subject_type: str, subjects, limit: int = 0):
        """A candidate list per subject — what a retrieval or ranking step returns, its own top-K for
        each user: for each of ``subjects``, which of *its own* candidate resources
        ``candidates[offsets[s]:offsets[s + 1]]`` it may see (HAS or CONDITIONAL) — with ``limit``, the
        first ``limit`` of them in its candidates' order. Returns ``((row_off, ids), err)``:
        ``ids[row_off[s]:row_off[s + 1]]`` are subject s's permitted candidates, both device tensors,
        selected and compacted by kernels over the finished plane (Engine.filter_groups_ids); only two
        count words come back to the host, and a per-item error — or malformed offsets — is ``err``.
        Parsing, retry and error mapping are ``FilterCrossDevice``'s."""
        return self._filter_groups("FilterGroupsDevice", ctx, cs, permission, subject_type, subjects, offsets, candidates,
                                   VARY_RESOURCE, limit)

    def FilterGroupSubjectsDevice(self, ctx: Optional[Context], cs: Optional[Strategy], resource_permission: str,
                                  resources, subject_type: str, candidates, offsets, limit: int = 0):
        """``FilterGroupsDevice``'s mirror: for each of ``resources``, which of *its own* candidate
        subjects ``candidates[offsets[r]:offsets[r + 1]]`` may see it. Returns ``((row_off, ids), err)``,
        ``ids[row_off[r]:row_off[r + 1]]`` the permitted candidate subjects of resource r."""
        return self._filter_groups("FilterGroupSubjectsDevice", ctx, cs, resource_permission, subject_type, resources,
                                   offsets, candidates, VARY_SUBJECT, limit)

    # ---- snapshot plumbing (ReadSchema + ExportRelationships at its revision) -------------
    def LoadSnapshot(self, schema: str, revision: int, relationships: Iterable) -> None:
        """Ingest the output of ``ReadSchema`` (client/client.go:416-422) and
        ``ExportRelationships`` at that revision (client/client.go:472-499)."""
        self.engine.load_schema(schema)
        lines = "\n".join(r.String() if hasattr(r, "String") else str(r) for r in relationships)
        self.engine.load_snapshot_text(revision, lines)

    def SetHeadRevision(self, revision: int) -> None:
        """The source's head revision that ``consistency.Full()`` must reach (consistency/
        consistency.go:25-35): ReadSchema's ReadAt token (client/client.go:416-422) or a Watch
        checkpoint. Until ApplyUpdates reaches it, a Full check is Unavailable and retried."""
        self.engine.set_head_revision(revision)

    _UPDATE_OPS = {_rel.UpdateCreate: "CREATE", _rel.UpdateTouch: "TOUCH", _rel.UpdateDelete: "DELETE"}

    def ApplyUpdates(self, revision: int, updates: Iterable) -> None:
        """Fold one Watch response into the local snapshot: the ``rel.Update`` values that
        ``UpdatesSinceRevision`` yields (client/client.go:370-413, rel/relationship.go:291-301)
        up to the response's ChangesThrough revision (which gochugaru's iterator drops; the
        caller passes it here). ``UpdateUnknown`` is rejected, as SpiceDB never sends it."""
        lines = []
        for u in updates:
            op = self._UPDATE_OPS.get(u.UpdateType)
            if op is None:
                raise InvalidArgument(f"unknown update type {u.UpdateType!r}")
            lines.append(op + " " + u.Relationship.String())
        self.engine.apply_updates_text(revision, "\n".join(lines))
