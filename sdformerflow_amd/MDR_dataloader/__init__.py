"""The event front end of the reference's MDR_dataloader (MVSEC / MDR), on the GPU: loader_utils.EventSequence and
loader_utils.EventSequenceToVoxelGrid_Pytorch.  File readers and augmentors are out of scope."""
