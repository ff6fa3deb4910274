"""Records tests/golden/reads_front.json: what a caller sees of the front of the read-batch calls (tests/helpers/reads_front.py)
on THIS build -- the library of the tree, or the one SASSY_HIP_LIBRARY names.  Run on the commit whose behaviour is to be kept:

  python tools/record_reads_front.py no_device <commit hash> [path]   anywhere; the calls run in a child that sees no device
  python tools/record_reads_front.py device <commit hash> [path]      on a device

Each run replaces its own part of the file and keeps the other."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))


def main():
    part, commit = sys.argv[1], sys.argv[2]
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "tests", "golden", "reads_front.json")
    assert part in ("no_device", "device"), part
    if part == "no_device" and os.environ.get("HIP_VISIBLE_DEVICES") != "-1":
        env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
        raise SystemExit(subprocess.call([sys.executable] + sys.argv, env=env))
    import sassy_amd
    import reads_front
    whole = json.load(open(out)) if os.path.exists(out) else {}
    whole[part] = {"recorded_on_commit": commit, "devices_when_recorded": sassy_amd.device_count() if part == "device" else 0}
    if part == "no_device":
        whole[part]["refusals"] = reads_front.no_device(sassy_amd)
    else:
        whole[part].update(reads_front.device(sassy_amd))
    with open(out, "w") as f:
        f.write("{\n")
        for i, (name, body) in enumerate(sorted(whole.items())):
            f.write(" %s: {\n" % json.dumps(name))
            keys = list(body)
            for j, key in enumerate(keys):
                last = "" if j + 1 == len(keys) else ","
                if isinstance(body[key], list):
                    f.write("  %s: [\n" % json.dumps(key) + ",\n".join("   " + json.dumps(e, separators=(",", ":")) for e in body[key]) + "\n  ]%s\n" % last)
                else:
                    f.write("  %s: %s%s\n" % (json.dumps(key), json.dumps(body[key]), last))
            f.write(" }%s\n" % ("" if i + 1 == len(whole) else ","))
        f.write("}\n")
    print("recorded", part, {k: len(v) for k, v in whole[part].items() if isinstance(v, list)}, "->", out)


if __name__ == "__main__":
    main()
