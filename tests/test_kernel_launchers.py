"""The launchers between the host and the kernels (etlg_k_* in etl_amd/csrc): every one host_state.h declares is defined once and
called by somebody, and every kernel of the hand-off units is launched by a launcher that somebody calls. Text only: no compiler, no GPU.

On the commit before this file the three checks report the launchers etlg_k_col_fixed and etlg_k_col_var — declared and defined, named by
nobody since the host took the pack forms — and the kernels only they launched: k_col_fixed, k_col_lens<false>, k_col_lens<true>,
k_col_copy, k_col_fmt<false> and k_col_fmt<true> (four names, six kernels; 82 272 code bytes in profiles/codec_split_codegen.txt). The second
check reports a third name there as well: etlg_k_copy_cells_table_bytes, a sizing helper of cells.hip that nothing called."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from etl_amd import build  # noqa: E402

CSRC = os.path.join(ROOT, "etl_amd", "csrc")
HANDOFF_UNITS = ["columns.hip", "rowformats.hip", "rowformats_dl.hip", "finish.hip", "check.hip", "fingerprint.hip"]
HOST_FILES = ["host.cpp", "host_control.inc", "host_decode.inc", "host_handoff.inc", "host_handoff_columns.inc", "host_handoff_rows.inc", "host_orchestrate.inc"]


def _read(csrc, name):
    return open(os.path.join(csrc, name)).read()


def _close(text, i, o, c):
    """Index behind the bracket that closes the one at text[i]."""
    depth = 0
    for k in range(i, len(text)):
        depth += (text[k] == o) - (text[k] == c)
        if depth == 0:
            return k + 1
    raise AssertionError("unbalanced " + o)


def declared(csrc):
    return sorted(set(re.findall(r'^extern "C" [^;]*?\b(etlg_k_\w+)\s*\(', _read(csrc, "host_state.h"), re.M)))


def definitions(text):
    """name -> [(start, end)] of every etlg_k_* function body in `text` (a name, its parameter list, then a brace)."""
    out = {}
    for m in re.finditer(r"\b(etlg_k_\w+)\s*\(", text):
        end = _close(text, m.end() - 1, "(", ")")
        rest = re.match(r"\s*\{", text[end:])
        if rest:
            brace = end + rest.end() - 1
            out.setdefault(m.group(1), []).append((m.start(), _close(text, brace, "{", "}")))
    return out


def unnamed_launchers(csrc):
    """Declared launchers that no host file (other than host_state.h) and no OTHER kernel source names."""
    texts = {f: _read(csrc, f) for f in HOST_FILES + [s for s in build.SOURCES if s not in HOST_FILES]}
    out = []
    for name in declared(csrc):
        home = [f for f in build.SOURCES if name in definitions(texts[f])]
        users = [f for f, t in texts.items() if f not in home and re.search(r"\b%s\b" % name, t)]
        if not users:
            out.append(name)
    return out


def unlaunched_kernels(csrc, unit, dead):
    """__global__ kernels in the text of a unit (the source and the project headers it includes) that no hipLaunchKernelGGL outside the
    bodies of the `dead` launchers names."""
    text = "\n".join(_read(csrc, f) for f in [unit] + build.headers_of(unit))
    kernels = set(re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(", text))
    assert kernels and len(kernels) == len(re.findall(r"__global__", text)), unit   # (every kernel's head has the shape the pattern reads)
    defs = definitions(text)
    for name in dead:
        for a, b in defs.get(name, []):
            text = text[:a] + " " * (b - a) + text[b:]
    launched = set(re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*(?:etlg::)?(\w+)", text))
    return sorted(kernels - launched)


def test_every_declared_launcher_is_defined_once():
    texts = {s: _read(CSRC, s) for s in build.SOURCES}
    names = declared(CSRC)
    assert len(names) > 40, names
    for name in names:
        homes = [(s, len(definitions(t).get(name, []))) for s, t in texts.items() if name in definitions(t)]
        assert len(homes) == 1 and homes[0][1] == 1, (name, homes)


def test_every_declared_launcher_is_called():
    assert unnamed_launchers(CSRC) == []


def test_every_handoff_kernel_is_launched():
    dead = unnamed_launchers(CSRC)
    for unit in HANDOFF_UNITS:
        assert unit in build.SOURCES
        assert unlaunched_kernels(CSRC, unit, dead) == [], unit


def test_job_launchers_take_typed_pointers():
    """No launcher takes its job as `const void*`: passing another job's struct does not compile."""
    for line in _read(CSRC, "host_state.h").split("\n"):
        if line.startswith('extern "C"') and "etlg_k_" in line:
            assert "void*" not in line.replace("void* scratch", ""), line
