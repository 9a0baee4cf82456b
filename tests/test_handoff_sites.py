"""Every cross-stream handoff in the engine carries the ordering tests' spin hook.

tests/test_gpu_ordering.py makes a missing wait fail deterministically by queueing a spin kernel on
a stream after each of its cross-stream waits (so what it produces next starts late) and before
each event another stream or host thread waits on (the test hook "handoff_spin",
include/scde_hip.h).  That only covers the handoffs that call the hook, so this check reads
the library's host code -- engine.hip (the pipeline) and engine_posterior.hip (one posterior), which
hold every handoff today, the feature files api_*.hip and the header they share: each `hipEventRecord` is either one of the
profiling marks (timing events of one stream, never waited on by another) or is immediately
preceded by a `handoff_spin(...)` on the same stream, and every `hipStreamWaitEvent` sits inside
`handoff_wait`, which spins after the wait.  A new handoff added without the hook, in any of
these files, fails here.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scde_amd", "csrc")
ENGINE = os.path.join(CSRC, "engine.hip")
HOST_FILES = ["engine_internal.h"] + sorted(f for f in os.listdir(CSRC)
                                            if re.fullmatch(r"engine\w*\.hip|api_\w+\.hip", f))


def _sources():
    for name in HOST_FILES:
        yield name, open(os.path.join(CSRC, name)).read()


def _records(lines):
    for i, line in enumerate(lines):
        m = re.search(r"hipEventRecord\(([^,]+),\s*([^)]+)\)", line)
        if m:
            yield i, m.group(1).strip(), m.group(2).strip()


def test_every_cross_stream_event_is_preceded_by_the_spin_hook():
    nrecs = 0
    missing = []
    for name, src in _sources():
        lines = src.split("\n")
        for i, ev, stream in _records(lines):
            nrecs += 1
            if ev in ("a", "b") and "(void)" in lines[i]:  # mark_begin / mark_end timing events
                continue
            prev = lines[i - 1]
            m = re.search(r"handoff_spin\(([^,]+),\s*([^)]+)\)", prev)
            if not m or m.group(2).strip() != stream:
                missing.append(f"{name}:{i + 1}: hipEventRecord({ev}, {stream}) without handoff_spin on {stream}")
    assert nrecs >= 14, nrecs  # the pipelined host path's handoffs (and the two timing marks)
    assert not missing, "\n".join(missing)


def test_every_cross_stream_wait_goes_through_handoff_wait():
    src = open(ENGINE).read()
    m = re.search(r"\n(?:static )?hipError_t (?:scde::host::)?handoff_wait\([^)]*\)\s*\{(.*?)\n\}", src, re.S)
    assert m, "handoff_wait helper missing"
    body = m.group(1)
    assert "hipStreamWaitEvent" in body and "handoff_spin" in body
    assert body.index("hipStreamWaitEvent") < body.index("handoff_spin")  # spin after the wait
    raw, nwaits = [], 0
    for name, text in _sources():
        rest = text[: m.start()] + text[m.end():] if name == "engine.hip" else text
        raw += [f"{name}:{text[: text.index(l)].count(chr(10)) + 1}: {l.strip()}"
                for l in rest.split("\n") if "hipStreamWaitEvent(" in l]
        nwaits += text.count("handoff_wait(") + text.count("lane_join(")
    assert not raw, "raw waits outside handoff_wait:\n" + "\n".join(raw)
    assert nwaits >= 16


def test_spin_hook_is_reachable_from_the_api():
    src = open(ENGINE).read()
    assert '"handoff_spin"' in src and "spin_cycles" in src and '"skip_lane_join"' in src
    hdr = open(os.path.join(ROOT, "include", "scde_hip.h")).read()
    assert "handoff_spin" in hdr and "scde_ctx_inject_fault" in hdr
