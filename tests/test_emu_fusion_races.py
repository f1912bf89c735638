"""CPU (host emulator): the decision logic of the four fusion races of yolov5_amd/engine.py -- Bottleneck + cv3 (Y5_FUSED_CV3), 3x3 + pointwise
(Y5_FUSED_K3PW), the fused front (Y5_FUSED_FRONT) and the fused Detect head (Y5_FUSED_HEAD) -- with y5_plan_time_range answered from a script: the
emulator's clock means nothing (every interval is 0 ms, so no fused form ever wins there).  Checked for each, through op_names, plan_table() and conv_cfgs: the
fused form is kept when it is STRICTLY faster than the launches it replaces and not otherwise; a refused fused op leaves the plain form without an exception;
mode 0 never times anything; mode 1 fuses with the iteration counts the engine documents.  For the two fusions that come in two builds (34 / 81, 56 / 87):
the faster build wins, a tie keeps the first, the choice lands in the tile-choice cache as (cfg, -1) under its mark, and a later engine times that build only.
The model and shapes are those at which tests/test_emu_bneck.py, test_emu_k3pw.py, test_emu_front.py and test_emu_head.py reach each fusion."""
import ctypes as C

import pytest
import torch

from tests.hipemu.backend import EmuBackend
from tests.test_emu_model import det_model
import yolov5_amd.engine as eng_mod
from yolov5_amd.engine import Engine

REFUSED = -2
FUSED_ADD = {"y5_plan_add_bottleneck_cv3": "cv3", "y5_plan_add_conv_k3pw": "k3pw", "y5_plan_add_conv_front": "front", "y5_plan_add_detect_head": "head"}
TWO_LAUNCH = {("y5_plan_add_bottleneck", "y5_plan_add_conv"): "cv3", ("y5_plan_add_conv", "y5_plan_add_conv"): "k3pw",
              ("y5_plan_add_conv", "y5_plan_add_detect_decode"): "head"}


class _Lib:
    """The real library with y5_plan_time_range scripted.  script[kind] = (fused ms, two-launch ms); for k3pw / head the fused entry is {build: ms}; for front
    the two-launch entry is (stem ms, 3x3 + pointwise ms).  A scratch plan of one op timed over [0, 1) is a fused form, of two ops over [0, 2) a two-launch form;
    a longer plan is the engine's own (the front's opponents).  A scratch plan's range runs once first, as the real call's warm-up does: a shape the library
    refuses (the fused head of the 2 x 4 level) is refused here too.  timed: (kind, form, build, iterations) of every call; refuse: fused adds answered with -2."""

    def __init__(self, lib, script, refuse=()):
        self._lib, self._script, self._refuse = lib, script, refuse
        self._ops, self._cfg, self.timed = {}, {}, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("y5_plan_add_"):
            return fn

        def add(plan, *args):
            if FUSED_ADD.get(name) in self._refuse:
                return REFUSED
            rc = fn(plan, *args)
            if rc == 0:
                self._ops.setdefault(plan.value, []).append(name)
                if name in ("y5_plan_add_conv_k3pw", "y5_plan_add_detect_head"):
                    self._cfg[plan.value] = int(args[0]._obj.cfg)    # the descriptor it saw
            return rc

        return add

    def y5_plan_destroy(self, plan):
        self._ops.pop(plan.value, None)    # (the allocator hands the address out again)
        self._cfg.pop(plan.value, None)
        return self._lib.y5_plan_destroy(plan)

    def y5_plan_time_range(self, plan, first, last, iters, st, ms):
        ops, size = self._ops.get(plan.value, []), self._lib.y5_plan_size(plan)
        build = None
        if size <= 2:    # the warm-up run of the real call: where the library refuses a shape
            rc = self._lib.y5_plan_run_range(plan, first, last, st)
            if rc != 0:
                return rc
        if size == 1 and (first, last) == (0, 1):
            kind, form = FUSED_ADD[ops[0]], "fused"
            t = self._script[kind][0]
            if isinstance(t, dict):
                build = self._cfg[plan.value]
                t = t[build]
        elif size == 2 and (first, last) == (0, 2):
            kind, form = TWO_LAUNCH[tuple(ops)], "two"
            t = self._script[kind][1]
        else:
            assert size > 2 and last == first + 1, (size, first, last)
            kind, form = "front", "k3pw" if first == 2 else "stem"
            t = self._script["front"][1][first == 2]
        self.timed.append((kind, form, build, iters))
        ms._obj.value = t
        return 0


class _Backend(EmuBackend):
    autotune = True

    def __init__(self, script, refuse=()):
        super().__init__()
        self.lib = _Lib(self.lib, script, refuse)


@pytest.fixture()
def clean_cache():
    eng_mod._TUNE_CACHE.clear()
    eng_mod._TUNE_FILE_STATE["loaded"] = False
    yield
    eng_mod._TUNE_CACHE.clear()
    eng_mod._TUNE_FILE_STATE["loaded"] = False


@pytest.fixture(scope="module")
def model():
    return det_model("yolov5s", 0, True).half()


MODES = {"cv3": "Y5_FUSED_CV3", "k3pw": "Y5_FUSED_K3PW", "front": "Y5_FUSED_FRONT", "head": "Y5_FUSED_HEAD"}
SHAPE = {"cv3": (1, 3, 64, 64), "k3pw": (1, 3, 64, 64), "front": (2, 3, 64, 64), "head": (1, 3, 64, 128)}
# what the fused plan shows in op_names and what it shows in its place otherwise
FUSED_NAMES = {"cv3": ["bneck+cv3:2.C3.m0+2.C3.cv3", "conv:2.C3.cv3(fused)"], "k3pw": ["conv+pw:1.Conv+2.C3.cv1+cv2", "conv:2.C3.cv1+cv2(fused)"],
               "front": ["front:0.Conv+1.Conv+2.C3.cv1+cv2"],
               "head": ["conv+decode:detect.m0", "decode0(fused)", "conv+decode:detect.m1", "decode1(fused)"]}
PLAIN_NAMES = {"cv3": ["bneck:2.C3.m0", "conv:2.C3.cv3"], "k3pw": ["conv:1.Conv", "conv:2.C3.cv1+cv2"], "front": [],
               "head": ["conv:detect.m0", "decode0", "conv:detect.m1", "decode1"]}
BUILDS = {"k3pw": (34, 81), "head": (56, 87)}
MARK = {"k3pw": eng_mod._K3PW_MARK, "head": eng_mod._HEAD_MARK}
RACES = {"cv3": 1, "k3pw": 1, "front": 1, "head": 2}     # how many ops of the plan reach the race (the Detect levels 0 and 1; level 2 is refused by the library when it runs)


def _script(kind, fused, two):
    """Every other race of the plan loses by a mile, so that only `kind` decides."""
    s = {"cv3": (9.0, 1.0), "k3pw": ({34: 9.0, 81: 9.0}, 1.0), "front": (9.0, (0.5, 0.5)), "head": ({56: 9.0, 87: 9.0}, 1.0)}
    s[kind] = (fused, two)
    return s


def _engine(monkeypatch, tmp_path, model, kind, mode, script, refuse=()):
    monkeypatch.setenv("Y5_TUNE_CACHE", str(tmp_path / "tune.json"))
    for k in ("Y5_DISABLE", "Y5_EXPERIMENTAL", "Y5_TUNE_RANK"):
        monkeypatch.delenv(k, raising=False)
    for k, var in MODES.items():
        monkeypatch.setenv(var, "0")
    if kind == "front":
        monkeypatch.setenv("Y5_FUSED_K3PW", "1")     # the front builds on the 3x3 + pointwise launch (tests/test_emu_front.py)
    if mode is None:
        monkeypatch.delenv(MODES[kind])              # auto is the default
    else:
        monkeypatch.setenv(MODES[kind], mode)
    monkeypatch.setattr(eng_mod, "autotune_conv", lambda lib, d, ptrs, st, exclude=(): -1)    # no tile race
    eng_mod._LAST_RACE[:] = [None, None]
    be = _Backend(script, refuse)
    eng = Engine(model, SHAPE[kind], torch.float16, "cpu", want_raw=False, backend=be)
    return eng, [t for t in be.lib.timed if t[0] == kind]


def _assert_form(eng, kind, fused, build=None):
    names, table = eng.op_names, eng.plan_table()
    assert [n for n in names if n in FUSED_NAMES[kind]] == (FUSED_NAMES[kind] if fused else []), names
    assert [n for n in names if n in PLAIN_NAMES[kind]] == ([] if fused else PLAIN_NAMES[kind]), names
    assert len(table) == len(names) and [n for n, _ in table] == names
    cfgs = {n: c for n, c in table}
    if kind == "front":
        assert (eng._front is not None) == fused
        if fused:
            assert cfgs[FUSED_NAMES[kind][0]] == "front" and names[eng._front] == FUSED_NAMES[kind][0] and eng._front == eng._stem + 1
        # what a forward on an fp16 NCHW batch launches: the front, then the plan from op 4 -- or the stem, then the plan from op 2
        eng._stem_active = True
        eng.time_ops(iters=1)
        assert eng.timed_order == ([eng._front] + list(range(4, eng._stem)) if fused else [eng._stem] + list(range(2, eng._stem)))
        return
    if kind == "cv3":
        assert (cfgs[FUSED_NAMES[kind][0]], cfgs[FUSED_NAMES[kind][1]]) == ("bneck", -2) if fused else cfgs["bneck:2.C3.m0"] == "bneck" and cfgs["conv:2.C3.cv3"] == -1
    elif kind == "k3pw":
        assert (cfgs[FUSED_NAMES[kind][0]], cfgs[FUSED_NAMES[kind][1]]) == (build, -2) if fused else cfgs["conv:1.Conv"] == -1 and cfgs["conv:2.C3.cv1+cv2"] == -1
    else:
        assert eng._fused_heads == ({0, 1} if fused else set())
        assert sorted(i for _, i in eng._anchor_ops) == [0, 1, 2]
        for lvl in (0, 1):
            assert cfgs[f"conv+decode:detect.m{lvl}" if fused else f"conv:detect.m{lvl}"] == (build if fused else -1)
    assert -2 not in eng.conv_cfgs or fused


# (fused ms, two-launch ms, fused kept): strictly faster only
DECISIONS = [(1.0, 2.0, True), (2.0, 1.0, False), (1.0, 1.0, False)]


def _times(kind, fused, two):
    if kind in BUILDS:
        fused = {b: fused for b in BUILDS[kind]}
    if kind == "front":
        two = (two * 0.5, two * 0.5)    # (exact in fp32: the engine adds the two)
    return fused, two


@pytest.mark.parametrize("kind", list(MODES))
@pytest.mark.parametrize("fused_ms,two_ms,kept", DECISIONS, ids=["faster", "slower", "equal"])
def test_auto_keeps_the_fused_form_only_when_strictly_faster(monkeypatch, tmp_path, clean_cache, model, kind, fused_ms, two_ms, kept):
    eng, timed = _engine(monkeypatch, tmp_path, model, kind, None, _script(kind, *_times(kind, fused_ms, two_ms)))
    _assert_form(eng, kind, kept, BUILDS.get(kind, (None,))[0])
    if kind == "front":
        assert timed == [("front", "fused", None, 10), ("front", "stem", None, 10), ("front", "k3pw", None, 10)]
    elif kind == "cv3":
        assert timed == [("cv3", "fused", None, 10), ("cv3", "two", None, 10)]
    else:
        a, b = BUILDS[kind]
        assert timed == [(kind, "fused", a, 10), (kind, "fused", b, 10), (kind, "two", None, 10)] * RACES[kind]


@pytest.mark.parametrize("kind", list(MODES))
def test_a_refused_fused_op_keeps_the_plain_form(monkeypatch, tmp_path, clean_cache, model, kind):
    for mode in (None, "1"):
        eng, timed = _engine(monkeypatch, tmp_path, model, kind, mode, _script(kind, *_times(kind, 1.0, 2.0)), refuse=(kind,))
        _assert_form(eng, kind, False)
        assert timed == []
        assert not [k for k in eng_mod._TUNE_CACHE if k[0] == MARK.get(kind)]


@pytest.mark.parametrize("kind", list(MODES))
def test_mode_0_never_fuses_and_never_times(monkeypatch, tmp_path, clean_cache, model, kind):
    eng, timed = _engine(monkeypatch, tmp_path, model, kind, "0", _script(kind, *_times(kind, 1.0, 2.0)))
    _assert_form(eng, kind, False)
    assert timed == []
    if kind != "front":
        assert eng.be.lib.timed == []


@pytest.mark.parametrize("kind", list(MODES))
def test_mode_1_fuses_with_the_documented_iteration_counts(monkeypatch, tmp_path, clean_cache, model, kind):
    """cv3: one iteration; front: not timed; k3pw / head: ten per build while the build is unknown, one of the known build afterwards; never the two-launch form."""
    eng, timed = _engine(monkeypatch, tmp_path, model, kind, "1", _script(kind, *_times(kind, 2.0, 1.0)))
    _assert_form(eng, kind, True, BUILDS.get(kind, (None,))[0])
    if kind == "front":
        assert timed == []
    elif kind == "cv3":
        assert timed == [("cv3", "fused", None, 1)]
    else:
        a, b = BUILDS[kind]
        assert timed == [(kind, "fused", a, 10), (kind, "fused", b, 10)] * RACES[kind]
        eng2, timed2 = _engine(monkeypatch, tmp_path, model, kind, "1", _script(kind, *_times(kind, 2.0, 1.0)))
        _assert_form(eng2, kind, True, a)
        assert timed2 == [(kind, "fused", a, 1)] * RACES[kind]


@pytest.mark.parametrize("kind", list(BUILDS))
@pytest.mark.parametrize("first_ms,second_ms,winner", [(1.0, 1.5, 0), (1.5, 1.0, 1), (1.0, 1.0, 0)], ids=["first", "second", "tie"])
def test_the_faster_build_wins_and_is_remembered(monkeypatch, tmp_path, clean_cache, model, kind, first_ms, second_ms, winner):
    a, b = BUILDS[kind]
    script = _script(kind, {a: first_ms, b: second_ms}, 2.0)
    eng, timed = _engine(monkeypatch, tmp_path, model, kind, None, script)
    _assert_form(eng, kind, True, BUILDS[kind][winner])
    marks = {k: v for k, v in eng_mod._TUNE_CACHE.items() if k[0] == MARK[kind]}
    assert len(marks) == RACES[kind] and all(v == (BUILDS[kind][winner], -1) for v in marks.values()), marks
    assert not [k for k in eng_mod._TUNE_CACHE if k[0] in MARK.values() and k[0] != MARK[kind]]
    # a later process: the choice comes back from the cache file, and only that build is timed
    eng_mod._TUNE_CACHE.clear()
    eng_mod._TUNE_FILE_STATE["loaded"] = False
    eng2, timed2 = _engine(monkeypatch, tmp_path, model, kind, None, script)
    _assert_form(eng2, kind, True, BUILDS[kind][winner])
    assert timed2 == [(kind, "fused", BUILDS[kind][winner], 10), (kind, "two", None, 10)] * RACES[kind]
    assert {k: v for k, v in eng_mod._TUNE_CACHE.items() if k[0] == MARK[kind]} == marks


@pytest.mark.parametrize("kind", list(BUILDS))
def test_the_build_is_remembered_even_when_the_fused_form_loses(monkeypatch, tmp_path, clean_cache, model, kind):
    a, b = BUILDS[kind]
    eng, _ = _engine(monkeypatch, tmp_path, model, kind, None, _script(kind, {a: 3.0, b: 2.5}, 2.0))
    _assert_form(eng, kind, False)
    marks = [v for k, v in eng_mod._TUNE_CACHE.items() if k[0] == MARK[kind]]
    assert marks == [(b, -1)] * RACES[kind]
