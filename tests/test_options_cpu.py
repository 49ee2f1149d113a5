"""The tuning options of libflooder_hip.so (csrc/flood_options.def) through flooder_set_option / flooder_get_option: every
name, its default and exactly the values it accepts.  No GPU: the library loads without one and the two entry points
touch no device.

TABLE below is this test's OWN copy of the option list, written down from the sources before the options moved into
flood_options.def - it is deliberately not derived from that file.  A new option needs a row here too."""
import json
import os
import re
import subprocess
import sys

from flooder_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX = 2**31 - 1   # INT_MAX: no upper probe

# name: (default, (lowest, highest)) or (default, [accepted values])
TABLE = {
    "bvh_grid": (1024, (1, 65536)),
    "bvh_ks": (0, [0, 1, 2, 4, 8]),
    "bvh_leaf_batch": (1, [1, 4]),
    "bvh_refine_pct": (100, (1, MAX)),
    "bvh_subs": (16, [1, 2, 4, 8, 16, 32, 64]),
    "cell_brute_max": (160, (0, MAX)),
    "cell_chunk_major": (1, (0, 2)),
    "cell_chunks_per_block": (12, (1, MAX)),
    "cell_density_grid": (16, (0, MAX)),
    "cell_drop": (1, (0, 1)),
    "cell_exh_dense": (32768, (512, MAX)),
    "cell_exh_sparse": (1920, (480, MAX)),
    "cell_exh_tries": (3, (0, 8)),
    "cell_grid": (1024, (1, 65536)),
    "cell_listed_first": (1, (0, 1)),
    "cell_min_grid": (384, (1, MAX)),
    "cell_one_pass": (125, (0, 100000)),
    "cell_queue_block": (5, (-1, 12)),
    "cell_retry_keep": (200, (0, MAX)),
    "cell_retry_pct": (50, (0, MAX)),
    "cell_split_launches": (1, (1, 2)),
    "cell_super_min_chunks": (49152, (0, MAX)),
    "cell_super_n0": (480, (0, MAX)),
    "cell_super_sparse": (600, (0, MAX)),
    "cell_super_weight": (2000, (0, MAX)),
    "cell_surface_pct": (60, (0, 100)),
    "cell_tail_waves": (200, (0, MAX)),
    "cell_tiles": (0, (0, 2)),
    "cell_tries": (2, (1, 8)),
    "cell_weight_classes": (1, (0, 1)),
    "curve": (1, (0, 1)),
    "curve_bits": (0, (0, 21)),
    "finish_budget": (14, (0, MAX)),
    "finish_budget_min": (64, (1, MAX)),
    "finish_focus_pct": (99, (0, 100)),
    "finish_items_cap": (65536, (1024, MAX)),
    "finish_order": (1, (0, 1)),
    "finish_refresh": (16, (1, MAX)),
    "finish_top": (0, (0, 1)),
    "finish_wide_points": (4194304, (0, MAX)),
    "fps_lane_best": (0, (0, 1)),
    "fps_rounds": (0, (0, 1)),
    "fps_rpl": (0, [0, 1, 4]),
    "fps_switch": (0, (0, MAX)),
    "sort_shape": (0, (0, 3)),
    "sorted_batch_pct": (400, (100, MAX)),
    "sorted_blocks": (0, (0, MAX)),
    "sorted_ks": (1, (1, 2)),
    "sorted_refresh": (4, (1, MAX)),
    "sweep_variant": (0, (0, 1)),
    "wit_adaptive": (0, (0, 1)),
    "wit_cmax_ext_pct": (60, (1, 10000)),
    "wit_cmax_pct": (250, (10, 10000)),
    "wit_flags": (0, (0, MAX)),
    "wit_grid": (1024, (1, MAX)),
    "wit_max_eval": (768, (0, MAX)),
    "wit_max_in_pct": (8, (0, MAX)),
    "wit_max_leaves": (400, (1, MAX)),
    "wit_max_live_pct": (12, (0, 100)),
    "wit_max_open": (48, (0, MAX)),
    "wit_min_bins": (48, (1, 64)),
    "wit_runs": (1, (0, 1)),
    "wit_sorted_stage": (1, (0, 1)),
    "wit_surface_pct": (60, (0, 100)),
    "wit_weight": (800, (0, MAX)),
}
ERROR_TEXT = b"flooder_set_option: unknown option or value"


def probes(accepted):
    """(values that must be accepted, values that must be rejected) of one row."""
    if isinstance(accepted, list):
        return list(accepted), [v for v in range(min(accepted) + 1, max(accepted)) if v not in accepted]
    lo, hi = accepted
    return [lo, hi], [lo - 1] + ([hi + 1] if hi != MAX else [])


def check_options(lib_path):
    """Runs in the child process: every failed check as a line of text (none: all is well)."""
    import ctypes

    lib = ctypes.CDLL(lib_path)
    lib.flooder_set_option.restype, lib.flooder_set_option.argtypes = _native.SIGNATURES["flooder_set_option"]
    lib.flooder_get_option.restype, lib.flooder_get_option.argtypes = _native.SIGNATURES["flooder_get_option"]
    lib.flooder_last_error.restype = ctypes.c_char_p
    E_ARG, bad = -1, []

    def get(name):
        v = ctypes.c_int(-12345)
        rc = lib.flooder_get_option(name.encode(), ctypes.byref(v))
        if rc != 0:
            bad.append(f"flooder_get_option({name}) returned {rc}")
        return v.value

    def refused(name, value, what):
        rc = lib.flooder_set_option(name, value)
        if rc != E_ARG or lib.flooder_last_error() != ERROR_TEXT:
            bad.append(f"{what}: returned {rc}, error text {lib.flooder_last_error()!r}")

    for name, (default, _) in TABLE.items():   # (all defaults first: setting one option must not move another)
        if get(name) != default:
            bad.append(f"{name}: default {get(name)}, expected {default}")
    for name, (default, accepted) in TABLE.items():
        good, wrong = probes(accepted)
        now = default
        for v in good:
            rc = lib.flooder_set_option(name.encode(), v)
            if rc != 0 or get(name) != v:
                bad.append(f"{name} = {v}: returned {rc}, value then {get(name)}")
            else:
                now = v
            for w in wrong:
                refused(name.encode(), w, f"{name} = {w}")
                if get(name) != now:
                    bad.append(f"{name} = {w} was refused but the value went from {now} to {get(name)}")
        if lib.flooder_set_option(name.encode(), default) != 0 or get(name) != default:
            bad.append(f"{name}: could not put the default {default} back")
    for name, (default, _) in TABLE.items():
        if get(name) != default:
            bad.append(f"{name}: {get(name)} after the probes of the other options, expected {default}")
    refused(b"no_such_option", 1, "unknown name")
    refused(None, 1, "NULL name")
    refused(b"cell_chunk_major_max", 262144, "cell_chunk_major_max")
    refused(b"", 1, "empty name")
    v = ctypes.c_int(-12345)
    for name, arg, what in ((b"no_such_option", ctypes.byref(v), "unknown name"), (None, ctypes.byref(v), "NULL name"),
                            (b"cell_chunk_major_max", ctypes.byref(v), "cell_chunk_major_max"),
                            (b"bvh_grid", None, "NULL value")):
        if lib.flooder_get_option(name, arg) != E_ARG or v.value != -12345:
            bad.append(f"flooder_get_option, {what}: not refused")
    return bad


def test_every_option_has_its_default_and_accepts_exactly_its_values():
    """In a fresh child process (this file run as a script): the options are process-wide."""
    assert os.path.exists(_native.LIB_PATH), "libflooder_hip.so not built (python -m flooder_amd.build)"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), _native.LIB_PATH]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    bad = json.loads(p.stdout.strip().split("\n")[-1])
    assert not bad, "\n".join(bad[:40])


def test_the_table_file_lists_exactly_these_options():
    text = open(os.path.join(ROOT, "flooder_amd", "csrc", "flood_options.def")).read()
    names = re.findall(r"^FLOODER_OPTION(?:_LIST)?\(\s*(\w+)", text, re.M)
    assert len(names) == len(set(names)), "an option is listed twice"
    assert set(names) == set(TABLE), (sorted(set(names) - set(TABLE)), sorted(set(TABLE) - set(names)))


def test_get_option_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "flooder_hip.h")).read()
    assert "int flooder_get_option(const char* name, int* value);" in header
    assert "flooder_get_option" in _native.SIGNATURES


if __name__ == "__main__":
    print(json.dumps(check_options(sys.argv[1])))
