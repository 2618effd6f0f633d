"""A table of PointCloud2 record layouts for the general record loader (load_f32 / load_ring, record_time): every ring
datatype in both byte orders, records of 13, 15, 29, 32 and 48 bytes, fields at odd offsets and in any order.  A layout is
filled from a canonical PointXYZIR cloud, so the expected result is the oracle's on that cloud whatever the layout."""
from dataclasses import dataclass

import numpy as np

from lidar_feature_extraction_amd import binding as B

RING_NUMPY = {B.INT8: "i1", B.UINT8: "u1", B.INT16: "i2", B.UINT16: "u2", B.INT32: "i4", B.UINT32: "u4"}
RING_NAME = {B.INT8: "int8", B.UINT8: "uint8", B.INT16: "int16", B.UINT16: "uint16", B.INT32: "int32", B.UINT32: "uint32"}
TIME_NUMPY = {B.FLOAT32: "f4", B.FLOAT64: "f8", B.UINT32: "u4"}


@dataclass(frozen=True)
class RecordLayout:
    name: str
    step: int
    x: int
    y: int
    z: int
    ring: int
    ring_type: int
    big_endian: bool
    time: int = -1                # offset of a time field, -1: none
    time_type: int = 0

    def fields(self):
        """The message's field list, in the order of their offsets, with the fields a driver adds and the library skips."""
        f = [("x", self.x, B.FLOAT32, 1), ("y", self.y, B.FLOAT32, 1), ("z", self.z, B.FLOAT32, 1), ("ring", self.ring, self.ring_type, 1)]
        if self.time >= 0:
            f.append(("t", self.time, self.time_type, 1))
        return sorted(f, key=lambda e: e[1])

    def library_layout(self):
        from lidar_feature_extraction_amd import layout_from_fields
        lay = layout_from_fields(self.fields(), self.step, self.big_endian)
        assert (lay.point_step, lay.off_x, lay.off_y, lay.off_z, lay.off_ring, lay.ring_datatype, lay.big_endian) == (
            self.step, self.x, self.y, self.z, self.ring, self.ring_type, int(self.big_endian))
        return lay

    def time_field(self):
        from lidar_feature_extraction_amd import time_field_from_fields
        tf = time_field_from_fields(self.fields(), self.step, self.big_endian)
        assert (tf.source, tf.offset, tf.datatype, tf.big_endian) == (B.TIME_FROM_FIELD, self.time, self.time_type, int(self.big_endian))
        return tf

    def _put(self, raw, offset, values, kind):
        v = np.ascontiguousarray(values).astype((">" if self.big_endian else "<") + kind)
        raw[:, offset:offset + v.dtype.itemsize] = v.view(np.uint8).reshape(len(v), v.dtype.itemsize)

    def fill(self, cloud, ring_ids=None):
        """Records of this layout holding the canonical cloud's x, y, z and ring (or ring_ids, any integers the ring type
        holds), every other byte junk: an array of `step`-byte items."""
        n = len(cloud)
        raw = np.random.default_rng(self.step * 131 + self.ring).integers(0, 256, (n, self.step), dtype=np.uint8)
        for name, off in (("x", self.x), ("y", self.y), ("z", self.z)):
            self._put(raw, off, cloud[name], "f4")
        ids = np.asarray(cloud["ring"] if ring_ids is None else ring_ids, np.int64)
        self._put(raw, self.ring, ids, RING_NUMPY[self.ring_type])
        return np.ascontiguousarray(raw).reshape(-1).view("V%d" % self.step)

    def put_times(self, stored):
        """The bytes of the time field for values as stored (float32, float64 or uint32): [n, size] uint8."""
        v = np.ascontiguousarray(stored).astype((">" if self.big_endian else "<") + TIME_NUMPY[self.time_type])
        return v.view(np.uint8).reshape(len(v), v.dtype.itemsize)


def _table():
    out = []
    # 13 bytes, x0 y4 z8 ring12: the one-byte ring types (big-endian still swaps the floats)
    for t in (B.INT8, B.UINT8):
        for be in (False, True):
            out.append(RecordLayout("tight13", 13, 0, 4, 8, 12, t, be))
    # 15 bytes with a two-byte ring in front: at 0 (x, y, z at 3, 7, 11) and at 1, where every offset is odd
    out.append(RecordLayout("front15", 15, 3, 7, 11, 0, B.INT16, False))
    out.append(RecordLayout("front15", 15, 3, 7, 11, 0, B.UINT16, True))
    out.append(RecordLayout("odd15", 15, 3, 7, 11, 1, B.INT16, True))
    out.append(RecordLayout("odd15", 15, 3, 7, 11, 1, B.UINT16, False))
    # the canonical 32-byte geometry, where only the ring type (or the byte order) sends the record to the general loader
    for t in (B.INT8, B.UINT8, B.INT16, B.INT32, B.UINT32):
        out.append(RecordLayout("xyzir32", 32, 0, 4, 8, 20, t, False))
    for t in (B.UINT16, B.INT16, B.INT32, B.UINT32):
        out.append(RecordLayout("xyzir32", 32, 0, 4, 8, 20, t, True))
    # 48 bytes, fields in z, y, x order with junk between them
    out.append(RecordLayout("zyx48", 48, 40, 20, 12, 6, B.INT32, True))
    out.append(RecordLayout("zyx48", 48, 41, 22, 13, 30, B.UINT32, False))
    out.append(RecordLayout("zyx48", 48, 40, 20, 12, 10, B.UINT16, False))
    return out


LAYOUTS = _table()


def layout_id(lay):
    extra = "" if lay.time < 0 else "-t%d-%s" % (lay.time, TIME_NUMPY[lay.time_type])
    return "%s-ring%d-%s-%s%s" % (lay.name, lay.ring, RING_NAME[lay.ring_type], "be" if lay.big_endian else "le", extra)


def timed29(time_type, big_endian):
    """29 bytes, x1 y5 z9 ring13 (UINT16) t15: no field is aligned, and a FLOAT64 time straddles two 8-byte words."""
    return RecordLayout("timed29", 29, 1, 5, 9, 13, B.UINT16, big_endian, 15, time_type)
