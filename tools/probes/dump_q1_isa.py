"""Generated source + gfx950 ISA of the Q1 scan kernel (k_agg_jit) without a GPU:
    python tools/probes/dump_q1_isa.py /tmp/isa [--narrow]   ->  /tmp/isa/q1_jit.hip, /tmp/isa/q1_jit.s"""
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import jit_source  # noqa: E402  (the program is the source tool's: tools/jit_source.py)
from minispark_amd import hipspark as hs  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out = Path(args[0] if args else "/tmp/isa")
out.mkdir(parents=True, exist_ok=True)
lib = hs.load_library()
cols, low = jit_source.q1("--narrow" in sys.argv)
rc, text = jit_source.generate(lib, jit_source.agg_case("q1", "private", cols, low))
assert rc == 0, lib.hs_last_error()
(out / "q1_jit.hip").write_text(text)
subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value",
                f"-I{ROOT / 'minispark_amd' / 'csrc'}", f"-I{ROOT / 'include'}", "-S", "--cuda-device-only", "-o", str(out / "q1_jit.s"),
                str(out / "q1_jit.hip")], check=True)
print(out / "q1_jit.s")
