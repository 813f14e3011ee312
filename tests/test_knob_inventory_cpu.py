"""The table of environment settings (tests/knob_cases.py) against the sources, and the SpMV geometry cases against the restated tile
mappings.  No device: a new `getenv("KRYST_...")` without a row fails here with its name, and so does a row whose setting is gone, a
setting that is run nowhere under tests/, and a geometry case that would not reach the loop trip it is there for."""
import glob
import os
import re

import pytest

import knob_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kryst_amd", "csrc")
READ = re.compile(r'\b(?:getenv|env_[a-z_]+)\s*\(\s*(?:[A-Za-z_]\w*\s*,\s*)?"(KRYST_[A-Z0-9_]+)"')
ONCE = re.compile(r'static\s+const\s+[^;=]*=\s*\[\]\s*\{[^}]*?getenv\("(KRYST_[A-Z0-9_]+)"\)')
TAGS = re.compile(r'static constexpr const char\* TAG = "(\w+)"')


def _sources():
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.isfile(path) and path.endswith((".hip", ".h", ".cpp", ".hpp")):
            with open(path) as f:
                yield os.path.basename(path), f.read()


def scan():
    """-> (names read, names read once per process, whether the KRYST_BPC_ family is built, the TAG names)"""
    names, once, tags, family = set(), set(), set(), False
    for _, text in _sources():
        names.update(READ.findall(text))
        once.update(ONCE.findall(text))
        tags.update(TAGS.findall(text))
        family = family or '"KRYST_BPC_"' in text
    return names, once, family, tags


def _tests_text():
    """every file under tests/ but the table and this file"""
    out = {}
    for path in glob.glob(os.path.join(ROOT, "tests", "**", "*"), recursive=True):
        if os.path.isfile(path) and path.endswith((".py", ".cpp", ".sh")) and os.path.basename(path) not in ("knob_cases.py", os.path.basename(__file__)):
            with open(path) as f:
                out[os.path.relpath(path, ROOT)] = f.read()
    return out


def test_every_setting_read_has_a_row_and_every_row_is_read():
    names, _, family, tags = scan()
    assert len(names) > 80 and family and len(tags) > 40, (len(names), family, len(tags))      # the scan itself still finds the sources
    want = names | {KC.FAMILY}
    rows = [r.name for r in KC.ROWS]
    assert len(rows) == len(set(rows)), sorted(n for n in rows if rows.count(n) > 1)
    assert sorted(want - set(rows)) == [], "read in kryst_amd/csrc without a row in tests/knob_cases.py"
    assert sorted(set(rows) - want) == [], "rows in tests/knob_cases.py that no source reads"


def test_per_process_agrees_with_the_source_pattern():
    _, once, _, _ = scan()
    marked = {r.name for r in KC.ROWS if r.per_process}
    assert sorted(once - marked) == [], "read once per process (function-local static const) but not marked per_process"
    assert sorted(marked - once) == [], "marked per_process but read per call"


def test_rows_are_complete():
    for r in KC.ROWS:
        if r.cls == "not-run":
            assert r.reason and not r.values, r.name
        else:
            assert r.values and r.op and r.shape and r.reason is None, r.name
    # the per-process profiles name per-process rows only, and every one of the solver grid settings
    for env in KC.PROFILES.values():
        assert all(KC.BY_NAME[k].per_process for k in env), env
    assert all(any(k in env for env in KC.PROFILES.values()) for k in KC.PER_PROCESS_BPC + ("KRYST_NO_ARENA",))


def test_every_setting_that_runs_is_named_in_a_test():
    """named in a file under tests/, or set by a profile of knob_cases.PROFILES that tests/test_gpu_knobs.py hands to the worker"""
    text = _tests_text()
    by_profile = {k for env in KC.PROFILES.values() for k in env}
    assert "KC.PROFILES[profile]" in text["tests/test_gpu_knobs.py"]

    def named(name, t):
        return re.search(re.escape(name) + r"\b", t) is not None
    assert sorted(KC.TESTED_IN) == sorted(r.name for r in KC.ROWS if r.cls != "not-run")
    stale = [n for n, f in KC.TESTED_IN.items() if not (named(n, text.get(f, "")) or (n in by_profile and f == "tests/test_gpu_knobs.py"))]
    assert stale == [], "the file a row points at no longer names the setting"
    missing = [r.name for r in KC.ROWS if r.cls != "not-run" and r.name not in by_profile and not any(named(r.name, t) for t in text.values())]
    assert missing == [], "form / geometry / transport rows that no file under tests/ names"


def test_profiles_reach_what_they_are_there_for():
    """the per-process profiles at the assumed CU count: which passes stride, and that the high profile's grids are not the default ones"""
    for profile in KC.PROFILES:
        wrong = [what for what, holds in KC.profile_conditions(profile) if not holds]
        assert wrong == [], (profile, wrong)
    assert KC.ntiles_of(KC.WORKER_BIG ** 3) == 2073
    # every value of a per-process grid row is set by a profile, except where the row says the value selects nothing
    for k in KC.PER_PROCESS_BPC:
        assert set(KC.BY_NAME[k].values) <= {env[k] for env in KC.PROFILES.values() if k in env}, k


@pytest.mark.parametrize("case", KC.GEOMETRY_CASES, ids=KC.geometry_label)
def test_spmv_geometry_case_under_the_restated_mapping(case):
    nt = case["ntiles"]
    visits = KC.mapping(case)
    assert KC.visited_once(visits, nt), "a tile is skipped or visited twice"
    if case["trips"] == "many":
        assert KC.max_trips(visits) >= 2, "no workgroup takes a second trip"
    else:
        assert KC.max_trips(visits) == 1
    if case.get("grouped"):
        g = case.get("group", 1)
        assert KC.slots_past_the_end(visits) >= 1, "no slot falls past ntiles"
        assert nt % (8 * g) != 0


def test_every_mapping_value_has_a_case_with_a_second_trip():
    """A stream kernel's default grid hands every workgroup one slot, and so does the pattern kernel at one tile per workgroup: those cases
    are marked trips="one".  Every value of every mapping setting must still meet a second trip somewhere -- for the stream kernels in the
    cases at 537 tiles on one workgroup per CU -- except the two values that MEAN one trip."""
    one_trip_by_definition = {("KRYST_SPMV_PATTERN_TPW", "1"), ("KRYST_SPMV_BLOCKS_PER_CU", "2")}
    by_kernel = {}
    for c in KC.GEOMETRY_CASES:
        for kv in c["env"].items():
            by_kernel.setdefault((c["kernel"],) + kv, []).append(c["trips"])
    lacking = sorted(k for k, trips in by_kernel.items() if "many" not in trips and k[1:] not in one_trip_by_definition)
    assert lacking == []
    for name in ("KRYST_SPMV_SWIZZLE", "KRYST_SPMV_GROUP", "KRYST_SPMV_BLOCKS_PER_CU", "KRYST_SPMV_PATTERN_TPW", "KRYST_SPMV_STAGE_GROUP", "KRYST_SPMV_STAGE_T"):
        ran = {c["env"][name] for c in KC.GEOMETRY_CASES if name in c["env"]}
        assert ran >= set(KC.BY_NAME[name].values), name


def test_the_restated_mappings_notice_a_wrong_mapping():
    """the conditions above are not vacuous: a mapping that forgets the XCD term repeats tiles, one without the guard runs past the end"""
    assert not KC.visited_once({k: (None if t is None else t // 2) for k, t in KC.stream_map(10).items()}, 10)
    assert KC.visited_once(KC.stream_map(10, group=3), 10) and KC.slots_past_the_end(KC.stream_map(10, group=3)) == 14
    assert KC.max_trips(KC.stream_map(512, bpc=1)) == 2 and KC.max_trips(KC.stream_map(512, bpc=1, num_cu=304)) == 2
    assert KC.max_trips(KC.stream_map(537, group=8, bpc=1)) == 3
