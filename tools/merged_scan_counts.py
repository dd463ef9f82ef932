"""Decision counters of the merged-scan test problems (tests/test_gpu_merged_scan.py: COUNT_CASES), as stored in
tests/golden/merged_scan_counts.json.  The stored file holds the numbers of the library built from the commit BEFORE the merged scan
(commit 5f947a1), selected with PARTLS_LIB; run on the GPU box from the repository root:
    PARTLS_LIB=<that build's libpartls_hip.so> python tools/merged_scan_counts.py > tests/golden/merged_scan_counts.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import partls_amd
import test_gpu_merged_scan as M


class _Env:                                          # pytest's monkeypatch, as far as the test module uses it
    def setenv(self, k, v): os.environ[k] = v
    def delenv(self, k, raising=True): os.environ.pop(k, None)


print(json.dumps({"_produced": "tools/merged_scan_counts.py on an MI355X with the library of commit 5f947a1, the parent of the merged KKT scan "
                               "(PARTLS_LIB); pivots / vetoes / best_index of a full opt_sweep, default chain length and PARTLS_CHAIN_LEN=7",
                  "counts": M.counts(partls_amd.package(), _Env())}, indent=1))
