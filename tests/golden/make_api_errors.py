"""Regenerates tests/golden/api_errors.json: the type name and str() of the exception every case of tests/api_error_cases.py
raises.  These freeze the argument errors of the package's Python layer (which argument is found first, and what the message
says); tests/test_api_errors.py replays the list against the file.  A case that returns is a defect of the list: nothing is
written."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import api_error_cases   # noqa: E402

out, returned = {}, []
for name, fn in api_error_cases.cases():
    got = api_error_cases.record(fn)
    if got is None:
        returned.append(name)
    else:
        out[name] = {"type": got[0], "message": got[1]}
if returned:
    sys.exit("these cases raise nothing; api_errors.json is not written:\n  " + "\n  ".join(returned))
with open(os.path.join(HERE, "api_errors.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", len(out), "cases")
