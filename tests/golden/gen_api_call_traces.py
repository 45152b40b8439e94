"""Writes api_call_traces.json: the call traces of KLTTrackSequence and KLTTrackFeatures that tests/api_trace_cases.py describes, as
commit 8524b0b (the parent of the commit that made the post-track stages one chain) produced them.  No device is needed.

    python tests/golden/gen_api_call_traces.py          # rewrites the file from the tree it is run in

Entries are kept once in "strings"; a trace is a list of indices into it, and a sequence longer than six frames its entry count and
sha256 alone.  Recording again is only right when the calls are MEANT to change; the test wants them equal."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

RECORDED_ON = "8524b0b"


def main():
    import api_trace_cases as cases
    seq, feat = cases.record_all()
    # the stand-in library's slot state must make the third call of a case repeat its chain, for every stage that has an entry point
    for stage, entry in cases.STAGE_ENTRY.items():
        shown = [name for name, t in feat.items() if name.startswith(stage + "/") and cases.repeats_chain(t, entry)]
        assert shown, "no KLTTrackFeatures case shows %s behind a repeated tracker" % entry
    both = dict(("sequence:" + k, v) for k, v in seq.items())
    both.update(("features:" + k, v) for k, v in feat.items())
    strings, encoded = cases.encode(both)
    entries = sum(len(v) if isinstance(v, list) else v["entries"] for v in encoded.values())
    path = os.path.join(HERE, "api_call_traces.json")
    with open(path, "w") as f:
        json.dump({"recorded_on": RECORDED_ON, "cases": len(encoded), "entries": entries, "strings": strings, "traces": encoded}, f,
                  separators=(",", ":"))
        f.write("\n")
    print("%d cases, %d entries, %d distinct, %d bytes" % (len(encoded), entries, len(strings), os.path.getsize(path)))


if __name__ == "__main__":
    main()
