"""Kernel selection, checked without a GPU: tests/select_probe.hip runs the library's planner (kr_plan.hip) and launchers
against a launch plumbing that records, and every line it prints - the template instantiation, grid, block and LDS
bytes of each launch, rc / last_sim_path / last_overlap / last_waves_per_rod, the pointers the launch code fills in -
must equal the line the parent of the planner gave for the same case (tests/golden/selection_parent.txt.gz: the probe's
own lines; as text they are 3 MB, so they are kept compressed, the KR_MSWO_GT sections as the lines that differ from the
default run).  The predictor image a simulate call hands to its kernels is checked against the parent's rule, restated here.
The five table-family sources (table, bank, loads, boundary, key points) have lines of their own, "src ...", which also
print the source struct every launch received; tests/golden/selection_parent_sources.txt.gz holds those of the commit
whose five launchers the one launch body replaced."""
import gzip
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "selection_parent.txt.gz")
GOLDEN_SOURCES = os.path.join(ROOT, "tests", "golden", "selection_parent_sources.txt.gz")
RUNS = {"default": None, "KR_MSWO_GT=1": "1", "KR_MSWO_GT=0": "0"}

# the matrix of select_probe.hip (run_matrix), counted independently
N_DTYPE, N_SCHEME, N_DIAG = 2, 2, 2
FULL = N_DTYPE * 11 * 9 * N_SCHEME * N_DIAG * 6 * 3        # N x B x network x {simulate, step, residual}
OPTIONS = N_DTYPE * 3 * 2 * 10 * N_SCHEME * N_DIAG * 2 * 2  # N {40, 100, 400} x B {256, 1024} x 10 option values x {none, served} x {simulate, step}
PREV = N_DTYPE * 2 * 2
TABLE_BANK = N_DTYPE * 5 * 2 * N_SCHEME * 11 * (6 + 3)      # N x B {8, 2048} x 11 option values x (6 table networks + 3 bank shapes)
PREPARE = N_DTYPE * 2
N_CASES = FULL + OPTIONS + N_DTYPE + PREV + TABLE_BANK + PREPARE  # (N_DTYPE: B = 2048 with overlap = 0)
# ... and of its "src" lines (run_src_matrix): the table / bank matrix for {table, loads, boundary, key points} and the bank
N_SRC_CASES = N_DTYPE * 5 * 2 * N_SCHEME * 11 * (4 * 6 + 3)

# rows recorded from the parent (fp64 unless said; Euler, diagonal matrices, default options unless said)
PARENT_ROWS = [
    "f64,100,1024,E,d1,n0,sim | 0 2 1 1 | mso_sim_kernel<double,true,18,1> 256x256 154880 r1h0p0l0; ms_sim_kernel<double,true,0,18,false,1> 256x256 152320 r1h0p0l0",
    "f64,100,256,E,d1,n0,sim | 0 2 1 4 | mswo_sim_kernel<double,4,false> 256x256 114880 r0h0p0l0",
    "f64,100,512,E,d1,n0,sim | 0 2 1 2 | mswo_sim_kernel<double,2,false> 512x128 77440 r0h0p0l0",
    "f64,400,512,E,d1,n0,sim | 0 2 1 2 | mswo_sim_kernel<double,2,true> 512x128 77440 r0h0p0l0",
    "f64,100,256,E,d1,n1,sim | 0 2 0 4 | msw_sim_kernel<double,true,4,true,1,2> 256x256 80320 r0h1p0l0",
    "f64,100,512,E,d1,n1,sim | 0 2 0 2 | msw_sim_kernel<double,true,2,true,1,2> 512x128 40896 r0h1p0l0",
    "f64,100,1024,E,d1,n1,sim | 0 2 0 1 | ms_sim_kernel<double,true,0,18,true,1> 256x256 159744 r0h0p0l0",
    "f32,100,2048,E,d1,n0,sim | 0 2 1 1 | mso_sim_kernel<float,true,20,2> 512x256 80640 r1h0p0l0; ms_sim_kernel<float,true,0,20,false,1> 512x256 79360 r1h0p0l0",
    "f32,100,2048,E,d1,n0,sim,overlap=0 | 0 2 0 1 | ms_sim_kernel<float,true,0,20,false,2> 512x256 79360 r0h0p0l0",
    "f64,100,256,E,d0,n0,sim | 0 2 0 4 | msw_sim_kernel<double,false,4,false,1,0> 256x256 103296 r0h0p0l0",
    "f64,100,256,E,d1,n0,sim,msw_overlap=0 | 0 2 0 4 | msw_sim_kernel<double,true,4,false,1,0> 256x256 103296 r0h0p0l0",
    "f64,400,256,E,d1,n0,sim,msw_overlap=0 | 0 2 0 4 | msw_sim_kernel<double,true,4,false,1,1> 256x256 112896 r0h0p0l0",
    "f64,100,256,E,d1,n0,sim,waves_per_rod=1 | 0 2 1 1 | mso_sim_kernel<double,true,18,1> 64x256 154880 r1h0p0l0; ms_sim_kernel<double,true,0,18,false,1> 64x256 152320 r1h0p0l0",
    "f64,100,1024,R,d1,n0,sim | 0 2 0 1 | ms_sim_kernel<double,true,1,18,false,1> 256x256 152320 r0h0p0l0",
    "f64,9,8,E,d1,n0,sim | 0 2 1 1 | mso_sim_kernel<double,true,18,1> 2x256 67584 r1h0p0l0; ms_sim_kernel<double,true,0,18,false,1> 2x256 65024 r1h0p0l0",
]
# ... and where the persistent form does not apply (one launch per step: path 0 or 1)
PARENT_PER_STEP = ["f64,100,1024,R,d1,n1,sim", "f64,128,1024,E,d1,n0,sim", "f64,400,1024,E,d1,n0,sim", "f64,8,8,E,d1,n0,sim"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.fail("hipcc not found (the library itself is built with it)")


def _golden(path):
    """{section: lines}; the first line of the file names the parent commit."""
    runs, cur = {}, None
    with gzip.open(path, "rt") as f:
        first = f.readline()
        assert first.startswith("#") and "parent commit" in first, first
        for line in f:
            line = line.rstrip("\n")
            if line.startswith("["):
                cur = runs.setdefault(line[1:-1], [])
            elif not line.startswith("#"):
                cur.append(line)
    base = runs["default"]
    index = {l.split(" | ")[0]: i for i, l in enumerate(base)}
    assert len(index) == len(base), path
    for k in list(runs):
        if k != "default":  # (a section of differences)
            full = list(base)
            for l in runs[k]:
                full[index[l.split(" | ")[0]]] = l
            runs[k] = full
    return runs


@pytest.fixture(scope="module")
def probe_lines(tmp_path_factory):
    out = tmp_path_factory.mktemp("select_probe") / "select_probe"
    cmd = [_hipcc(), "-O0", "-std=c++17", "--cuda-host-only", "-rdynamic", "-w",
           "-I", os.path.join(ROOT, "knode-cosserat_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "select_probe.hip"), "-o", str(out), "-ldl", "-Wl,--unresolved-symbols=ignore-all"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = {}
    for name, gt in RUNS.items():
        env = {k: v for k, v in os.environ.items() if k != "KR_MSWO_GT"}
        if gt is not None:
            env["KR_MSWO_GT"] = gt
        r = subprocess.run([str(out)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
        lines[name] = [l for l in r.stdout.splitlines() if not l.startswith(("#", "pred ", "src "))]
        if gt is None:
            lines["pred"] = [l for l in r.stdout.splitlines() if l.startswith("pred ")]
            lines["src"] = [l for l in r.stdout.splitlines() if l.startswith("src ")]
    return lines


def test_matrix_is_complete(probe_lines):
    for name in RUNS:
        lines = probe_lines[name]
        assert len(lines) == N_CASES, (name, len(lines), N_CASES)
        labels = [l.split(" | ")[0] for l in lines]
        assert len(set(labels)) == N_CASES, name  # every combination is one line
    got = set(probe_lines["default"])
    for row in PARENT_ROWS:
        assert row in got, row
    by_label = {l.split(" | ")[0]: l for l in probe_lines["default"]}
    for label in PARENT_PER_STEP:
        rc, path = by_label[label].split(" | ")[1].split()[:2]
        assert rc == "0" and path in ("0", "1"), by_label[label]
        assert "step_kernel<" in by_label[label]


@pytest.mark.parametrize("run", list(RUNS))
def test_selection_equals_parent(probe_lines, run):
    want = _golden(GOLDEN)[run]
    got = probe_lines[run]
    assert len(want) == len(got) == N_CASES
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, "%d of %d lines differ; first:\nparent: %s\nnow:    %s" % (len(bad), N_CASES, bad[0][0], bad[0][1])
    assert not any("ARGS{" in l for l in got)  # a scalar member of SimArgs / StepArgs that did not arrive as passed


def test_sources_equal_parent(probe_lines):
    """Every table-family source through launch_sim: the selection and, per launch, the source struct the kernel received
    (table rows and N; the loads or boundary history; kp, K and both mask words; the bank's index array and stride, each
    a sentinel of its own) equal what the parent's five launchers gave."""
    want = _golden(GOLDEN_SOURCES)["default"]
    got = probe_lines["src"]
    assert len(want) == len(got) == N_SRC_CASES, (len(want), len(got), N_SRC_CASES)
    assert len({l.split(" | ")[0] for l in got}) == N_SRC_CASES  # every combination is one line
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, "%d of %d lines differ; first:\nparent: %s\nnow:    %s" % (len(bad), N_SRC_CASES, bad[0][0], bad[0][1])
    assert not any("ARGS{" in l for l in got)
    # every kind launches all three of its kernels somewhere, and every sentinel is seen where it belongs
    for kind, field in (("tab", "src{rows=0x12000 N=100}"), ("loads", "N=100 loads=0x20000}"), ("bnd", "N=100 bnd=0x30000}"),
                        ("kp", "N=100 bnd=0x30000 kp=0x50000 K=3 lo=100000005 hi=8000000000000002}")):
        mine = [l for l in got if l.startswith("src f64,100,") and l.split(" | ")[0].split(",")[6] == kind]
        launched = " ".join(l.split(" | ")[2] for l in mine if l.split(" | ")[1].startswith("0 "))
        assert "mso_sim_kernel<double,true,18,1,RodTable" in launched and ",false,1,RodTable" in launched and ",true,1,RodTable" in launched, kind
        assert all(field in part for l in mine if l.split(" | ")[1].startswith("0 ") for part in l.split(" | ")[2].split("; ")), kind
    bank = [l for l in got if l.startswith("src f32,9,8,E,d1,n1,bank | 0 ")]
    assert bank and "src{rows=0x11000 N=9 idx=0x60000 stride=256 layers=3}" in bank[0]


def test_forced_tile_placement_changes_the_plan(probe_lines):
    """KR_MSWO_GT is read: the three runs are not one run three times."""
    d, g1, g0 = (probe_lines[k] for k in RUNS)
    assert any(a != b for a, b in zip(d, g1)) and any(a != b for a, b in zip(d, g0))
    label = "f64,100,256,E,d1,n0,sim"
    pick = lambda ls: next(l for l in ls if l.startswith(label + " | "))
    assert "mswo_sim_kernel<double,4,false>" in pick(d) and "mswo_sim_kernel<double,4,true>" in pick(g1)


def test_predictor_image_follows_the_parents_rule(probe_lines):
    """plan_pred_image / note_sim_plan against simulate_impl of the parent commit: a persistent launch saves the image
    iff keep_predictor; per-step launches get it iff predictor > 2 and multiple shooting is wanted (ms_mode = 1, or
    auto and B <= ms_batch_limit) - whichever step kernel the plan names; never more than 1 GB of it; it is loaded iff
    keep_predictor and it was written for this B, W and network state; afterwards it is valid for this call's B
    (0 after single-shooting steps), W and network state, and untouched where the call did not use the buffer."""
    lines = probe_lines["pred"]
    assert len(lines) == 5 * 2 * 2 * 4 * 2 * 2 * 5
    seen = set()
    for line in lines:
        case, plan, image, after = line.split(" | ")
        kv = dict(f.split("=") for f in case.split()[1:])
        B, keep, valid = int(kv["B"]), int(kv["keep"]), int(kv["valid"])
        ms_mode = int(kv.get("ms_mode", -1))
        ms_wanted = ms_mode == 1 or (ms_mode != 0 and B <= int(kv.get("ms_batch_limit", 1 << 30)))
        path, W, nn = map(int, plan.split())
        wanted = keep == 1 if path == 2 else int(kv["predictor"]) > 2 and ms_wanted
        use = wanted and B * W * 24 * 64 * 8 <= 1 << 30
        load = use and keep == 1 and valid == 1
        before = (0 if valid == 0 else B + 1 if valid == 2 else B, (2 if W == 1 else 1) if valid == 3 else W, nn ^ (valid == 4))
        want_after = ((B if path else 0), W, nn) if use else before
        assert tuple(map(int, image.split())) == (use, B * W, load), line
        assert tuple(map(int, after.split())) == want_after, line
        seen.add((path, W > 1, use))
    # (the several-wavefront step kernel with and without the image, single shooting, the persistent forms)
    assert {(1, True, True), (1, True, False), (0, False, True), (2, True, True), (2, False, True), (2, False, False)} <= seen, seen
