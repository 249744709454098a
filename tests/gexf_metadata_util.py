"""What tests/test_gexf_metadata_host.py and tests/test_gpu_gexf_metadata.py share: the recorded exports with metadata of
tests/golden/gexf_metadata/ (made by tests/golden/make_gexf_metadata.py from the reference's own
export_to_GEXF(path, False, metadata[, False, False])) and a recorded case's metadata back as a mapping."""
import glob
import os

METADATA_FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gexf_metadata", "*.json")))


def metadata_of(rec):
    """{organism: ordered {attribute: value}} as the CLI holds it"""
    return {org: {title: value for title, value in pairs} for org, pairs in rec["metadata"]}


def read_text(path):
    return open(path, newline="", encoding="utf-8").read()
