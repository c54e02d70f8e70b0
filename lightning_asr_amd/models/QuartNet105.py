"""``MyModel2`` with the reference's ``QuartNet105`` encoder (models/QuartNet.py:175-224: ten residual blocks of five separable
convolutions), on the native HIP plan (variant "q105")."""
from ._base import MyModel2Base


class MyModel2(MyModel2Base):
    variant = "q105"
