"""The bytes of a built seed index, for tests that compare two builds of one genome
(test_index_build_gpu.py: CPU vs GPU builder; test_index_build_deterministic.py: thread counts)."""
import ctypes as C
import filecmp
import os

INDEX_FILES = ("GenomeIndex", "OverflowTable", "GenomeIndexHash", "Genome")


def image(idx):
    """-> dict: info() and the raw bytes of slots, tableBase, tableSize and overflow from view()."""
    info = idx.info()
    v = idx.view()
    nt = info["nHashTables"]
    return {
        "info": info,
        "slots": C.string_at(v.slots, 12 * info["totalHashSlots"]),
        "tableBase": C.string_at(v.tableBase, 8 * nt),
        "tableSize": C.string_at(v.tableSize, 8 * nt),
        "overflow": C.string_at(v.overflow, 4 * info["overflowTableSize"]) if info["overflowTableSize"] else b"",
    }


def assert_same_index(a, b, tmp_path=None):
    """a, b: GenomeIndex.  Equal info, byte-equal tables; with tmp_path also byte-equal save() files
    (the per-table `used` counts live only there)."""
    ia, ib = image(a), image(b)
    assert ia["info"] == ib["info"]
    for f in ("tableBase", "tableSize", "overflow", "slots"):
        if ia[f] != ib[f]:
            n = min(len(ia[f]), len(ib[f]))
            first = next((i for i in range(0, n, 4) if ia[f][i:i + 4] != ib[f][i:i + 4]), n)
            raise AssertionError(f"{f} differs: {len(ia[f])} vs {len(ib[f])} bytes, first at word {first // 4}")
    if tmp_path is not None:
        da, db = os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")
        a.save(da)
        b.save(db)
        for f in INDEX_FILES:
            assert filecmp.cmp(os.path.join(da, f), os.path.join(db, f), shallow=False), f
    return ia
